// The slot core of the pipelined ELBO calls: stage, enqueue and collect of one batch in a slot of a context, and where the slots'
// streams and child contexts come from.  vbmc_elbo_submit / collect (abi_elbo_slots.hip) and the multi-GPU submit / collect
// (abi_comm.hip) are built on it.
#pragma once
#include <algorithm>

#include "ctx_core.h"    // ctx_create_impl, null_gp_for
#include "elbo_pass.h"

// The slot's own pinned block stands in for the context's while this object lives: the inputs are staged in it and the copies enqueued
// against it, and the context's block is back in place on every way out.
struct SlotPinScope {
  vbmc_ctx* ctx; int slot;
  SlotPinScope(vbmc_ctx* c, int s) : ctx(c), slot(s) { swap(); }
  ~SlotPinScope() { swap(); }
  void swap() { std::swap(ctx->pin, ctx->slot_pin[slot]); std::swap(ctx->pin_cap, ctx->slot_pin_cap[slot]); }
};

// stage + enqueue + read-back of one batch into `slot` of the context, WITHOUT the event that marks its end (the caller may append work
// of its own to the stream first: the exchange of vbmc_elbo_multi_submit)
static vbmc_status elbo_submit_core(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* a, int slot, const char* who,
                                    bool allow_direct = false) {
  if (!a) return set_err(ctx, VBMC_ERR_INVALID, "%s: null args", who);
  if (slot < 0 || slot > 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: slot must be 0 or 1", who);
  if (ctx->slot_busy[slot]) return set_err(ctx, VBMC_ERR_INVALID, "%s: slot %d holds an uncollected pass", who, slot);
  if (a->separate_K || a->I_sk || a->J_sjk || a->G_s || a->varG_s || a->dG_s || a->dvarG_s)
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: per-component / per-hyper-sample outputs only through vbmc_elbo_batch", who);
  if (a->eps_mode == 1)
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: host-resident draws (eps_mode 1) only through vbmc_elbo_batch", who);
  if (!gp) {
    if (a->compute_var != 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: an entropy-only call (gp == NULL) has no variance", who);
    VB_TRY(null_gp_for(ctx, a->D, &gp));
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->slot_ev[slot]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->slot_ev[slot], hipEventDisableTiming));
  if (!ctx->slot_plan[slot]) ctx->slot_plan[slot] = new SlotPlan();
  SlotPlan* sp = (SlotPlan*)ctx->slot_plan[slot];
  sp->P = ElboPlan{};
  vbmc_status s_;
  {
    SlotPinScope pin(ctx, slot);
    s_ = elbo_plan(ctx, gp, a, sp->P, 0, true);
    // Result blocks of at most 256 KB are written by the finalize kernel straight into the pinned block (no read-back launch: BASELINE
    // configs[1] 52.1 -> 50.0 us per step, nothing elsewhere), only where nothing on the device reads the records afterwards (not under a
    // communicator: k_comm_pick does).  The mirror image -- the staging block read
    // by the pass's first kernel instead of a copy launch -- was built and measured too: no gain (49.8 us), removed.
    const size_t direct_kb = 256;
    if (!s_) {
      sp->hout = (double*)ctx->pin + sp->P.n_up;
      if (allow_direct && direct_kb && sp->P.compute_var == 0 && sp->P.out_n * sizeof(double) <= direct_kb * 1024) sp->P.out_direct = sp->hout;
    }
    if (!s_) s_ = elbo_enqueue(ctx, gp, sp->P, a->seed);
    if (!s_ && !sp->P.out_direct) s_ = elbo_enqueue_readback(ctx, sp->P, a, sp->hout);
  }
  if (s_) (void)hipStreamSynchronize(ctx->stream);   // nothing of a failed submit stays in flight
  return s_;
}
// ... and the event: the slot is busy from here on
static vbmc_status elbo_submit_mark(vbmc_ctx* ctx, int slot, const char* who) {
  ctx->slot_busy[slot] = true;
  hipError_t e_ = hipEventRecord(ctx->slot_ev[slot], ctx->stream);
  if (e_ != hipSuccess) {   // the pass is enqueued but cannot be waited for through the event: drain it and give the slot back
    (void)hipGetLastError();
    (void)hipStreamSynchronize(ctx->stream);
    ctx->slot_busy[slot] = false;
    return set_err(ctx, VBMC_ERR_HIP, "%s: hipEventRecord: %s", who, hipGetErrorString(e_));
  }
  return VBMC_OK;
}

// ---- where a new stream lands.  The runtime gives a stream a hardware queue, and the k-th hardware queue a process creates sits on
// dispatch pipe k mod 4 (tools/stream_pipes.hip, profiles/r04_experiments.md section 11): a kernel of a stream on the SAME pipe as a
// stream whose large grid is being handed out waits until the last workgroup of that grid is out -- for the entropy kernel ten
// elevenths of its duration -- and one on the same queue until it has finished.  Which queues exist when the slot streams are created
// is the process's history (torch, RCCL, other contexts), so the placement is measured: a candidate stream is kept if a one-wave
// kernel on it finishes early in the life of a long, low-occupancy kernel on each of the streams it has to run beside.
__global__ void k_place_probe(long long ticks) {
  extern __shared__ char probe_lds[];
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) { }
  if (ticks < 0) probe_lds[threadIdx.x] = 0;
}
// when the small kernel on `b` finished, as a fraction of the long kernel on `a` (both streams idle before); 2 on any error
static double place_ratio(int device, int num_cu, hipStream_t a, hipStream_t b) {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  double best = 2.0;
  bool ok = true;
  for (auto& ev : e) ok = ok && hipEventCreate(&ev) == hipSuccess;
  int khz = 100000;
  (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device);
  const long long ticks = (long long)(15e-6 * khz * 1e3);     // 15 us per workgroup, three rounds of four one-wave workgroups per compute unit
  for (int rep = 0; ok && rep < 2; ++rep) {
    ok = ok && hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess;
    ok = ok && hipEventRecord(e[0], a) == hipSuccess;
    hipLaunchKernelGGL(k_place_probe, dim3(num_cu * 12), dim3(64), 36 * 1024, a, ticks);
    hipLaunchKernelGGL(k_place_probe, dim3(1), dim3(64), 0, b, ticks / 50);
    ok = ok && hipEventRecord(e[1], b) == hipSuccess && hipEventRecord(e[2], a) == hipSuccess;
    ok = ok && hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess;
    float ts = 0.f, tl = 0.f;
    ok = ok && hipEventElapsedTime(&ts, e[0], e[1]) == hipSuccess && hipEventElapsedTime(&tl, e[0], e[2]) == hipSuccess;
    if (ok && tl > 0.f) best = std::min(best, (double)ts / tl);
  }
  for (auto& ev : e) if (ev) (void)hipEventDestroy(ev);
  if (!ok) (void)hipGetLastError();
  return ok ? best : 2.0;
}
// a new stream that dispatches beside every stream of `beside` (up to six candidates; the first one if none does)
static hipStream_t stream_beside(vbmc_ctx* ctx, const hipStream_t* beside, int nb, int priority = 0) {
  hipStream_t cand[6];
  int nc = 0;
  hipStream_t pick = nullptr;
  while (nc < 6 && !pick) {
    hipStream_t s = nullptr;
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority) != hipSuccess) { (void)hipGetLastError(); break; }
    cand[nc++] = s;
    bool ok = true;
    for (int i = 0; i < nb && ok; ++i) ok = place_ratio(ctx->device, ctx->num_cu, beside[i], s) < 0.35;
    if (ok) pick = s;
  }
  if (!pick && nc) pick = cand[0];
  for (int i = 0; i < nc; ++i)
    if (cand[i] != pick) (void)hipStreamDestroy(cand[i]);
  return pick;
}

// The context (and its slot) a pass submitted into public slot `slot` runs on: child context slot & 1, its slot slot >> 1 (see
// vbmc_ctx.slot_sub) for the optimiser-loop / sieve form of the call; this context itself, slots 0 and 1 only, for the variance forms
// (their lazily built per-surrogate blocks live in the parent's pool) and under VBMC_SLOT_STREAMS=0 (A/B runs).  The child's stream is
// ordered after everything enqueued on the parent's stream so far (a surrogate uploaded, draws produced there).
static vbmc_status slot_ctx(vbmc_ctx* ctx, const vbmc_elbo_args* a, int slot, vbmc_ctx** out, int* inner) {
  static const bool off = [] { const char* e = getenv("VBMC_SLOT_STREAMS"); return e && !strcmp(e, "0"); }();
  *out = ctx; *inner = slot;
  if (slot < 0 || slot >= VBMC_SLOTS) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_submit: slot must be 0 .. %d", VBMC_SLOTS - 1);
  if (off || ctx->is_sub || !a || a->compute_var != 0) {
    if (slot > 1) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_submit: slots 2 and 3 exist for passes without a variance term (and not under VBMC_SLOT_STREAMS=0)");
    return VBMC_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int ch = slot & 1;
  if (!ctx->slot_sub[0] || !ctx->slot_sub[1]) {     // both children at once, before anything runs on either: the second beside the first
    for (int c2 = 0; c2 < 2; ++c2) {
      if (ctx->slot_sub[c2]) continue;
      hipStream_t other = ctx->slot_sub[1 - c2] ? ctx->slot_sub[1 - c2]->stream : nullptr;
      hipStream_t s = stream_beside(ctx, &other, other ? 1 : 0);
      if (!s) return set_err(ctx, VBMC_ERR_HIP, "vbmc_elbo_submit: no stream for slot %d", slot);
      vbmc_ctx* sc = nullptr;
      vbmc_status st = ctx_create_impl(ctx->device, s, &sc, false);     // no fork on a slot stream (elbo_enqueue): one stream per child
      if (st != VBMC_OK) { (void)hipStreamDestroy(s); return set_err(ctx, st, "vbmc_elbo_submit: no stream for slot %d", slot); }
      sc->own_stream = true;
      sc->is_sub = true;
      ctx->slot_sub[c2] = sc;
    }
  }
  if (!ctx->slot_xev[slot]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->slot_xev[slot], hipEventDisableTiming));
  vbmc_ctx* sc = ctx->slot_sub[ch];
  sc->profiling = false;
  // ... when there is anything: an event recorded on an idle stream and waited for on another is still a device-side dependency between
  // two queues, 15-30 us per step where a step is that short (tools/archive/r4_host_cost.py: one restart at VBMC's own sample count 58 -> 27 us
  // per step, BASELINE configs[1] 89 -> 52).
  if (hipStreamQuery(ctx->stream) != hipSuccess) {
    (void)hipGetLastError();
    HIP_TRY(ctx, hipEventRecord(ctx->slot_xev[slot], ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(sc->stream, ctx->slot_xev[slot], 0));
  }
  *out = sc; *inner = slot >> 1;
  return VBMC_OK;
}
// an error of the child context reported through the parent the caller holds
static vbmc_status slot_err(vbmc_ctx* ctx, vbmc_ctx* sc, vbmc_status st) {
  if (st != VBMC_OK && sc != ctx) ctx->err = sc->err;
  return st;
}
static bool slot_in_flight(const vbmc_ctx* ctx, int slot) {
  return slot >= 0 && slot < VBMC_SLOTS && ctx->slot_where[slot] && ctx->slot_where[slot]->slot_busy[ctx->slot_inner[slot]] &&
         (ctx->slot_where[slot] != ctx || ctx->slot_inner[slot] == slot);
}

// waits for the pass submitted in `slot`; *sp_out: its plan and the pinned block its results landed in
static vbmc_status elbo_collect_core(vbmc_ctx* ctx, const vbmc_elbo_args* a, int slot, const SlotPlan** sp_out, const char* who) {
  if (!a || slot < 0 || slot > 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: null args / slot not 0 or 1", who);
  if (!ctx->slot_busy[slot]) return set_err(ctx, VBMC_ERR_INVALID, "%s: nothing submitted in slot %d", who, slot);
  const SlotPlan* sp = (const SlotPlan*)ctx->slot_plan[slot];
  // elbo_unpack copies T = plan.T doubles per restart into the caller's arrays: the layout must be the submitted one
  int T_now = 0;
  { const int n[4] = {a->D * a->K, a->K, a->D, a->K}; for (int g = 0; g < 4; ++g) if (a->optimize[g]) T_now += n[g]; }
  if (a->D != sp->P.dm.D || a->K != sp->P.dm.K || a->R != sp->P.dm.R || T_now != sp->P.dm.T ||
      (a->compute_grad ? 1 : 0) != sp->P.compute_grad)
    return set_err(ctx, VBMC_ERR_INVALID, "%s: args differ from the submitted ones (D, K, R, optimize flags, compute_grad)", who);
  ctx->slot_busy[slot] = false;
  hipError_t e_ = hipEventSynchronize(ctx->slot_ev[slot]);
  if (e_ != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, VBMC_ERR_HIP, "%s: %s", who, hipGetErrorString(e_)); }
  *sp_out = sp;
  return VBMC_OK;
}
