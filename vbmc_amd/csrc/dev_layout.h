// One description per packed block (host only, nothing of HIP): a layout accumulates the block as a running byte count, add<T>(n)
// names a window of it, and the block's size, the packing of its host image and the pointers into its device copy all come from
// those windows.  Windows are packed back to back, no padding.  A sub-block composes as add(sub): a window of sub.bytes() bytes
// whose at(base) is the base of the sub-layout's own windows.
#pragma once
#include <cstddef>
#include <cstring>

template <class T>
struct DevWin {
  size_t off = 0, n = 0;   // bytes from the block's base; elements
  bool present = true;     // absent: at() gives nullptr (the space is kept if n > 0)
  T* at(void* base) const { return present ? (T*)((char*)base + off) : nullptr; }
  const T* at(const void* base) const { return present ? (const T*)((const char*)base + off) : nullptr; }
  size_t size() const { return n * sizeof(T); }
  size_t end() const { return off + size(); }
  DevWin part(size_t first, size_t count) const { return DevWin{off + first * sizeof(T), count, present}; }   // elements [first, first + count)
  // copy a host array into the image of the block at this window (nothing for an absent window or a null source)
  void put(void* image, const T* src) const { if (present && src && n) memcpy(at(image), src, size()); }
};

struct DevLayout {
  size_t nbytes = 0;
  template <class T> DevWin<T> add(size_t n, bool present = true) {   // present = false: absent, its n elements reserved all the same
    DevWin<T> w{nbytes, n, present};
    nbytes += n * sizeof(T);
    return w;
  }
  template <class T> DevWin<T> add_if(bool present, size_t n) { return add<T>(present ? n : 0, present); }   // absent takes no space
  DevWin<unsigned char> add(const DevLayout& sub) { return add<unsigned char>(sub.nbytes); }
  void round_up(size_t unit) { nbytes = (nbytes + unit - 1) / unit * unit; }
  size_t bytes() const { return nbytes; }
  template <class T = double> size_t count() const { return nbytes / sizeof(T); }   // the size in elements of a block of one type
};
