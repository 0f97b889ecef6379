// C-ABI entry point of the marginal total variation: vbmc_vp_mtv (include/vbmc_hip.h).  The kernels are mtv_kernels.h; the packing of
// a posterior and the split of a draw are vp_tools_host.h's; everything from the draws to the integral is mtv_host.h's MtvPipeline,
// here over two runs whose draws are held together, with the mesh cut at each posterior's bounds, the caller's random blocks, and
// k_mtv_dct as the cosine transform.
// Here: validation, the two posteriors' uploads and the one pair (0, 1).
// vbmc_vp_corner, the data of a corner plot (cornerplot.m's histograms and kde2d densities, quantile1's quantiles), is corner_host.h's
// CornerPipeline over corner_kernels.h; here its refusal order and the choice between a posterior's draws and a caller's matrix.
#include "corner_host.h"
#include "mtv_host.h"
#include "vp_tools_host.h"

extern "C" vbmc_status vbmc_vp_mtv(vbmc_ctx* ctx, const vbmc_vp_desc* vp1, const vbmc_vp_desc* vp2, const vbmc_mtv_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_vp_mtv";
  if (!args || args->struct_size != sizeof(vbmc_mtv_args)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  MtvPipeline kde;
  VB_TRY(kde.begin(ctx, who, "posterior", *args));
  VptPack pk[2];
  VB_TRY(vpt_pack(ctx, who, vp1, 0.0, pk[0]));
  VB_TRY(vpt_pack(ctx, who, vp2, 0.0, pk[1]));
  if (vp1->D != vp2->D) return set_err(ctx, VBMC_ERR_INVALID, "%s: the posteriors have D = %d and D = %d", who, vp1->D, vp2->D);
  const int D = vp1->D;
  VB_TRY(kde.alloc(2, D, pk, true, true));
  const vbmc_vp_desc* vps[2] = {vp1, vp2};
  const double* blocks[2] = {args->block1, args->block2};
  double* xx[2] = {args->xx1, args->xx2};
  VptGenHost g[2];
  for (int s = 0; s < 2; ++s) {
    VB_TRY(vpt_gen_host(ctx, who, vps[s]->K, vps[s]->w, args->Ns, 1, args->seed + (uint64_t)s, g[s]));
    g[s].G.origflag = 1;
    VB_TRY(vpt_upload(ctx, pk[s]));
    VB_TRY(vpt_gen_upload(ctx, who, D, blocks[s], g[s]));
    VB_TRY(kde.add_run(s, pk[s], g[s], xx[s]));
  }
  VB_TRY(kde.finish(false, *args));
  if (!args->mtv) return VBMC_OK;
  std::vector<double> v;
  VB_TRY(kde.integrals({0, 1}, v));
  std::copy(v.begin(), v.end(), args->mtv);
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_vp_corner(vbmc_ctx* ctx, const vbmc_vp_desc* vp, const vbmc_corner_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_vp_corner";
  if (!args || args->struct_size != sizeof(vbmc_corner_args)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  CornerPipeline cp;
  VB_TRY(cp.begin(ctx, who, vp != nullptr, *args));
  if (!vp) {
    VB_TRY(cp.alloc(args->D, *args));
    VB_TRY(cp.upload(args->X_in));
    return cp.finish(*args);
  }
  VptPack pk;
  VB_TRY(vpt_pack(ctx, who, vp, 0.0, pk));
  VB_TRY(cp.alloc(vp->D, *args));
  VptGenHost g;
  VB_TRY(vpt_gen_host(ctx, who, vp->K, vp->w, args->Ns, args->balanceflag, args->seed, g));
  g.G.origflag = args->origflag ? 1 : 0;
  VB_TRY(vpt_upload(ctx, pk));
  VB_TRY(vpt_gen_upload(ctx, who, vp->D, args->block, g));
  VB_TRY(cp.draw(pk, g));
  return cp.finish(*args);
}
