// C-ABI entry points of libvbmc_hip.so for streams of independent ELBO batches (include/vbmc_hip.h): submit enqueues a pass into one of
// four slots and returns, collect waits for it.  The slot core is elbo_slots.h; abi_comm.hip builds its multi-GPU submit / collect on it too.
#include "elbo_slots.h"

extern "C" vbmc_status vbmc_elbo_submit(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* a, int slot) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (slot_in_flight(ctx, slot)) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_submit: slot %d holds an uncollected pass", slot);
  vbmc_ctx* sc = ctx;
  int inner = slot;
  VB_TRY(slot_ctx(ctx, a, slot, &sc, &inner));
  { vbmc_status s_ = elbo_submit_core(sc, gp, a, inner, "vbmc_elbo_submit", true); if (s_) return slot_err(ctx, sc, s_); }
  ctx->slot_where[slot] = sc; ctx->slot_inner[slot] = inner;
  ctx->last_ent_form = sc->last_ent_form; ctx->last_lj_form = sc->last_lj_form;    // (a child context's pass: vbmc_ctx_last_launch asks this one)
  return slot_err(ctx, sc, elbo_submit_mark(sc, inner, "vbmc_elbo_submit"));
}

extern "C" vbmc_status vbmc_elbo_collect(vbmc_ctx* ctx, const vbmc_elbo_args* a, int slot) {
  if (!ctx) return VBMC_ERR_INVALID;
  const SlotPlan* sp = nullptr;
  if (slot < 0 || slot >= VBMC_SLOTS) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_collect: slot must be 0 .. %d", VBMC_SLOTS - 1);
  if (!slot_in_flight(ctx, slot)) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_collect: nothing submitted in slot %d", slot);
  vbmc_ctx* sc = ctx->slot_where[slot];
  { vbmc_status s_ = elbo_collect_core(sc, a, ctx->slot_inner[slot], &sp, "vbmc_elbo_collect"); if (s_) return slot_err(ctx, sc, s_); }
  elbo_unpack(sp->P, a, sp->hout);
  return VBMC_OK;
}

// gives a slot back without its results: waits for the pass in flight (if any) and clears the slot -- for a caller that will not collect
// (an exception between submit and collect, an abandoned generator).  No-op on an idle slot.
extern "C" vbmc_status vbmc_elbo_abandon(vbmc_ctx* ctx, int slot) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (slot < 0 || slot >= VBMC_SLOTS) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_abandon: slot must be 0 .. %d", VBMC_SLOTS - 1);
  if (!slot_in_flight(ctx, slot)) return VBMC_OK;
  vbmc_ctx* sc = ctx->slot_where[slot];
  const int inner = ctx->slot_inner[slot];
  hipError_t e_ = sc->slot_ev[inner] ? hipEventSynchronize(sc->slot_ev[inner]) : hipStreamSynchronize(sc->stream);
  sc->slot_busy[inner] = false;
  if (e_ != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, VBMC_ERR_HIP, "vbmc_elbo_abandon: %s", hipGetErrorString(e_)); }
  return VBMC_OK;
}
