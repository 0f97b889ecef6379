"""CPU check of vbmc_amd/csrc/dev_layout.h, the one description of a packed block: a stand-alone program (its own main, the header
its only project include, no HIP) built by the host C++ compiler with the address and undefined-behaviour sanitizers and run.  It
checks that windows of mixed element sizes lie back to back, that a zero-count window takes no space, that an absent window is a null
pointer (with and without its space kept), that a composed sub-layout lands where its window says, that bytes() is the last window's
end, and that writing the last element of every window of a heap image of bytes() bytes is clean under the sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "dev_layout.h"

static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); bad = 1; } } while (0)

int main() {
  // mixed element sizes, back to back, no padding
  DevLayout L;
  DevWin<double> a = L.add<double>(3);
  DevWin<int> b = L.add<int>(5);
  DevWin<unsigned char> c = L.add<unsigned char>(7);
  DevWin<long long> d = L.add<long long>(2);
  CHECK(a.off == 0 && a.end() == 24);
  CHECK(b.off == 24 && b.end() == 44);
  CHECK(c.off == 44 && c.end() == 51);
  CHECK(d.off == 51 && d.end() == 67);
  CHECK(L.bytes() == 67 && L.bytes() == d.end());
  // a zero-count window takes no space
  DevWin<double> z = L.add<double>(0);
  CHECK(z.off == 67 && z.end() == 67 && L.bytes() == 67);
  // absent without space, absent with its space kept, and present through add_if
  DevWin<double> gone = L.add_if<double>(false, 9);
  CHECK(gone.n == 0 && L.bytes() == 67);
  DevWin<double> kept = L.add<double>(4, false);
  CHECK(kept.off == 67 && L.bytes() == 99);
  DevWin<int> there = L.add_if<int>(true, 3);
  CHECK(there.off == 99 && there.n == 3 && L.bytes() == 111);
  // a composed sub-layout: its windows resolve against the window it was added as
  DevLayout sub;
  DevWin<unsigned char> s0 = sub.add<unsigned char>(3);
  DevWin<double> s1 = sub.add<double>(2);
  CHECK(sub.bytes() == 19);
  DevWin<unsigned char> w = L.add(sub);
  DevWin<int> tail = L.add<int>(1);
  CHECK(w.off == 111 && w.size() == 19 && tail.off == 130 && L.bytes() == 134 && L.bytes() == tail.end());
  // rounding up to whole doubles, and the size in elements
  DevLayout R;
  R.add<unsigned char>(4 * 3);
  R.round_up(sizeof(double));
  CHECK(R.bytes() == 16 && R.count() == 2 && R.count<int>() == 4);
  R.round_up(sizeof(double));
  CHECK(R.bytes() == 16);
  // a part of a window
  DevWin<int> p = b.part(2, 3);
  CHECK(p.off == 32 && p.n == 3 && p.end() == b.end());

  // a heap image of exactly bytes(): every window's last element written, the pointers where the offsets say
  char* img = (char*)std::malloc(L.bytes());
  std::memset(img, 0, L.bytes());
  CHECK((char*)a.at(img) == img && (char*)b.at(img) == img + 24 && (char*)c.at(img) == img + 44 && (char*)d.at(img) == img + 51);
  CHECK(gone.at(img) == nullptr && kept.at(img) == nullptr && there.at(img) != nullptr);
  const char* cimg = img;
  CHECK(kept.at(cimg) == nullptr && (const char*)d.at(cimg) == cimg + 51);
  char* sb = (char*)w.at(img);
  CHECK(sb == img + 111 && (char*)s1.at(sb) == img + 114);
  // (a packed block holds doubles at odd byte offsets here on purpose: write them bytewise, as the copy helper does)
  const double one = 1.0; const long long two = 2; const int three[3] = {3, 3, 3}; const unsigned char seven[7] = {7, 7, 7, 7, 7, 7, 7};
  const double a3[3] = {1, 2, 3}; const int b5[5] = {1, 2, 3, 4, 5}; const long long d2[2] = {8, 9}; const double s2[2] = {5, 6};
  a.put(img, a3); b.put(img, b5); c.put(img, seven); d.put(img, d2); there.put(img, three); s1.put(sb, s2);
  s0.at(sb)[s0.n - 1] = 9;
  std::memcpy(img + tail.off, &three[0], sizeof(int));
  kept.put(img, a3);                       // absent: nothing is written
  gone.put(img, a3);
  a.put(img, nullptr);                     // a null source: nothing is written
  double back; long long back2; int back3;
  std::memcpy(&back, img + a.end() - 8, 8); CHECK(back == 3.0);
  std::memcpy(&back2, img + d.end() - 8, 8); CHECK(back2 == 9);
  std::memcpy(&back, img + w.off + s1.end() - 8, 8); CHECK(back == 6.0);
  std::memcpy(&back3, img + L.bytes() - 4, 4); CHECK(back3 == 3);
  std::memcpy(&back, img + kept.off, 8); CHECK(back == 0.0);
  CHECK((unsigned char)img[c.end() - 1] == 7 && (unsigned char)img[w.off + s0.end() - 1] == 9);
  (void)one; (void)two;
  std::free(img);
  std::printf(bad ? "dev_layout: FAILED\n" : "dev_layout: ok\n");
  return bad;
}
"""


def test_dev_layout_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(str(tmp_path), "dev_layout_check.cpp")
    exe = os.path.join(str(tmp_path), "dev_layout_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "dev_layout: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_dev_layout_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "dev_layout.h")).read()
    assert "hip" not in text.lower().replace("nothing of hip", ""), "dev_layout.h is host only"
