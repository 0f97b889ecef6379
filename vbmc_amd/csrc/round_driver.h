// The host loop that drives a device-resident chain in chunks of rounds, reading its progress one chunk behind: shared by the slice
// sampler and the train optimiser (abi_gp_train.hip), the acquisition search (abi_acq_search.hip) and the ensemble sampler (is_core.h).
#pragma once
#include <algorithm>

#include "common.h"

namespace {
// Chunks of rounds, the progress state (`bytes` at d_state) read one chunk behind the one being enqueued: it lands in one of two
// slots of ctx->pin, `stride` bytes apart, behind ev_fork / ev_join (these calls fork nothing onto the second stream).  classify
// reads a landed slot.  On a stall the rounds already enqueued are no-ops: the queue is drained, ONE checked round enqueued, and
// the read-behind starts again.
// (rounds enqueued behind the end of the chain, or behind a stall, launch nothing in propose / build / factorise / solve / decide,
// but k_gp_scale and k_nlz_final still run their workgroups: the chunks start at `first` = 4 rounds and double up to cap, so that
// a short chain wastes a handful of such rounds and a long one at most two chunks of them)
enum class Progress { running, finished, stalled };
template <class Round, class Classify>
vbmc_status drive_rounds(vbmc_ctx* ctx, const char* who, int cap, Round round, const void* d_state, size_t bytes, size_t stride, Classify classify,
                         int first = 4) {
  hipStream_t st = ctx->stream;
  hipEvent_t ev[2] = {ctx->ev_fork, ctx->ev_join};
  if (!ev[0] || !ev[1]) return set_err(ctx, VBMC_ERR_HIP, "%s: the context has no events", who);
  int k = 0, chunk = first;
  bool have_prev = false, finished = false;
  vbmc_status rs = VBMC_OK;
  while (!finished && rs == VBMC_OK) {
    for (int r = 0; r < chunk && rs == VBMC_OK; ++r) rs = round(0);
    chunk = std::min(2 * chunk, cap);
    if (rs != VBMC_OK) break;
    HIP_TRY(ctx, hipMemcpyAsync((char*)ctx->pin + (size_t)k * stride, d_state, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipEventRecord(ev[k], st));
    if (have_prev) {
      HIP_TRY(ctx, hipEventSynchronize(ev[k ^ 1]));
      const Progress p = classify((const char*)ctx->pin + (size_t)(k ^ 1) * stride);
      if (p == Progress::finished) finished = true;
      else if (p == Progress::stalled) {
        HIP_TRY(ctx, hipStreamSynchronize(st));     // the rounds behind a stall are no-ops: nothing to wait for but the queue
        rs = round(1);
        have_prev = false;
        k ^= 1;
        continue;
      }
    }
    have_prev = true;
    k ^= 1;
  }
  (void)hipStreamSynchronize(st);                    // whatever is still enqueued finds the work finished and does nothing
  return rs;
}
}  // namespace
