// Which kernels an ELBO pass runs and in what shape: decided ONCE per plan (plan_launch, called by elbo_plan in elbo_pass.h) from the shape
// and call facts, the device facts and the A/B switches.  elbo_enqueue only executes the LaunchChoice it finds in the plan.
#pragma once
#include <algorithm>
#include "elbo_kernels.h"

// The A/B switches of the launch decisions, read once per PLAN (not per process: the fuzz tool and the tests toggle them between two
// calls of one process; an in-process toggle takes effect on the next plan).  Every rule below takes this struct.
struct LaunchSwitches {
  enum Kernel { AUTO = 0, VALU, MFMA, LANE };
  Kernel ent_kernel = AUTO, lj_kernel = AUTO;   // VBMC_ENT_KERNEL = valu / mfma / lane, VBMC_LJ_KERNEL = valu / mfma: that kernel, also outside its class (A/B runs, tests)
  bool lj_co_off = false, walk_off = false, debug_occ = false;   // VBMC_LJ_CO=0: the log joint keeps its separate launch.  VBMC_ENT_WALK=0: the chunk grid.  VBMC_DEBUG_OCC: the chunk model's figures on stderr
  bool chunks_set = false;                      // VBMC_ENT_CHUNKS is set: A/B testing of the chunk model (no second chunk class, no walk) ...
  int chunks = 0, ent_hv = 0;                   // ... with this many chunks where the shape has that many tiles.  VBMC_ENT_HV: waves per workgroup where both splits fit
};
static LaunchSwitches read_launch_switches() {
  LaunchSwitches sw;
  auto kernel = [&](const char* e) { return !e ? sw.AUTO : !strcmp(e, "valu") ? sw.VALU : !strcmp(e, "mfma") ? sw.MFMA : !strcmp(e, "lane") ? sw.LANE : sw.AUTO; };
  auto off = [](const char* e) { return e && !strcmp(e, "0"); };
  sw.ent_kernel = kernel(getenv("VBMC_ENT_KERNEL")); sw.lj_kernel = kernel(getenv("VBMC_LJ_KERNEL"));
  sw.lj_co_off = off(getenv("VBMC_LJ_CO")); sw.walk_off = off(getenv("VBMC_ENT_WALK"));
  if (const char* e = getenv("VBMC_ENT_CHUNKS")) { sw.chunks_set = true; sw.chunks = atoi(e); }
  if (const char* e = getenv("VBMC_ENT_HV")) sw.ent_hv = atoi(e);
  sw.debug_occ = getenv("VBMC_DEBUG_OCC") != nullptr;
  return sw;
}
// The inputs of the decision.  The shape and the call (ElboPlan derives from it: elbo_plan fills these in first) ...
struct LaunchShape {
  ElboDims dm{};
  int compute_grad = 0, dt = 0;   // dt: the padded dimension of the DT-templated kernels
  int Mh = 0;                // antithetic sample pairs per component (0: the deterministic entropy bound, no Monte-Carlo launch)
  int Rp = 0, plan_restarts = 0;   // Rp: the restarts the launch shapes are chosen for -- R, or the undivided batch's, vbmc_elbo_args.plan_restarts (> 0: the chunking must be that launch's)
  int rstride = 1, eps_mode = 0;   // vbmc_elbo_args.restart_stride (device-RNG key stride of the restarts), vbmc_elbo_args.eps_mode
  int cw = 1;                // devices the entropy chunks are sharded over (the chunk model fills cw chips)
  bool lj_records = false, pipelined = false;   // the caller reads per-hyper-sample log-joint records (separate_K, G_s / varG_s, the variance kernels); a pass of vbmc_elbo_submit
  double cutoff = 0.0;       // > 0: the block-sparse entropy mode
};
// ... and the device and the context
struct LaunchDevice {
  int num_cu;
  bool prof_alone;    // vbmc_ctx_set_profiling(ctx, 2): nothing forked beside the dominant kernel
  vbmc_ctx* aux_of;   // ctx_aux(aux_of): is there an auxiliary stream to fork the log joint onto?  (creates it on first use)
  int (*mfma_occupancy)(int qs, int kt, int hv, bool grad, const EntArgs& ea);   // workgroups of an instantiation per compute unit (registers and LDS: hipOccupancyMaxActiveBlocksPerMultiprocessor)
  int (*lane_occupancy)(int D, int K, bool grad);
};
// The outcome (ElboPlan derives from it too; elbo_enqueue executes it)
struct LaunchChoice {
  int ent_form = 0, lj_form = 0;   // VBMC_ENTFORM_* / VBMC_LJFORM_* (vbmc_ctx_last_launch reports them where the kernel is really enqueued)
  bool use_mfma = false, use_lane = false;
  bool fork = false, lj_split = false;   // the log joint runs on the auxiliary stream beside the entropy kernel; separate VALU log joint: the training set split over four waves per cell
  int qs = 0, kt = 0, hv = 1;      // the matrix-core entropy instantiation (mfma_entropy_fits)
  int C = 1, tpc = 1;              // chunks per (component, restart), tiles per chunk
  int walk_tpw = 0, walk_nw = 0;   // > 0: the matrix-core entropy kernel WALKS (entropy_mfma.h): tiles per wave, waves of the launch
  int co_c1 = 0, co_c2 = 0, co_tpc2 = 0;   // co_c2 > 0: two chunk classes (EntArgs: the role's workgroups take the second, shorter one)
  int co_nsplit = 0, co_nwg = 0, co_rows = 0;   // the log-joint role (LjCo: splits of the training set, workgroups per restart, grid rows)
  bool role() const { return lj_form == VBMC_LJFORM_ROLE_MFMA || lj_form == VBMC_LJFORM_ROLE_LANE; }
};

#define ENT_LANE_WAVES_HOST 4     // = ENT_LANE_WAVES (entropy_lane.h)
// the role's staged inputs (entropy_lane.h: ent_lane_role_lds) must fit the launch's dynamic LDS; larger training sets keep the separate log-joint kernel
static bool lane_role_fits(int D, int K, int N, int S) {
  return ((size_t)((N + 63) & ~63) * (D + ENT_LANE_WAVES_HOST) + (size_t)S * GPC_STRIDE(D) + (size_t)VpLayout{D, K}.stride() + D) * sizeof(double) <= 48 * 1024;
}
// The class: K <= 16, D <= 12, dense -- minus the corner where the two signs' densities and the gradient accumulators of a lane do not
// fit 256 registers (DT = 12 with KP >= 10, DT = 10 with KP >= 12: built for one wave per SIMD those kernels take 2-3x the matrix-core
// kernel's time, tools/run_lane_sweep.sh; they are not instantiated).
static bool lane_entropy_fits(int D, int K, double cutoff) {
  const int dt = 2 * ((D + 1) / 2), kp = 2 * ((K + 1) / 2);
  return D >= 1 && D <= 12 && K >= 1 && K <= 16 && !(cutoff > 0.0) && !((dt >= 12 && kp >= 10) || (dt >= 10 && kp >= 12));
}
// ... and a batch wide enough to fill the chip with 64-sample tiles: a single chain (K R tiles < ~100) is bound by the launch's own
// latencies, where the matrix-core kernel's role splits the training set over more waves (6 % to 10 % faster there)
#define ENT_LANE_MIN_TILES 96
// Waves per workgroup for 64 < K <= 128 (tools/tune_sweep.py, round 2): two -- four are 10-30 % slower (more exchange and barrier
// coupling) -- EXCEPT where the two-wave kernel with four k-tiles per wave and a wide operand (D >= 15) spills its way down:
// there four waves with two k-tiles each fit their registers (D = 24, K = 128: 3.4 vs 5.7 ms; D = 20, K = 128: 3.9 vs 5.0;
// D = 20, K = 100 the other way: 50 vs 57 ms at configs[4]).
// K <= 64: one wave per workgroup.  Round 3 (tools/hv_small_sweep.py -> profiles/r03_hv_small.md) tried two waves with two k-tiles
// each where the one-wave kernel with four k-tiles spills: once those kernels were rebuilt for ONE wave per SIMD (512 registers,
// ent_one_wave_for in entropy_mfma.h: 11-23 % faster) the split only wins at K = 57..64 for D >= 31 (6 %) and costs 6-85 % everywhere else.
static int ent_hv_small(int qs, int K) { return (qs >= 9 && K > 52) ? 2 : 1; }   // (round 4, with the shared even part in the two-wave kernels: K = 53..56 at D >= 31 too, 0.77 of the one-wave time)
static int ent_hv_mid(int qs, int K) { return (K > 96 && (qs >= 7 || (qs >= 5 && K > 112))) ? 4 : 2; }
// K <= 64: one wave per (chunk, component, restart) with kt = ceil(K/16) k-tiles; larger mixtures split their components
// over the hv = 2 or 4 waves of a workgroup, kt = ceil(ceil(K/hv)/16) <= 4: two waves up to K = 128, four up to K = 256.
// VBMC_ENT_HV = 2 / 4 forces the split where both fit (A/B runs).  D <= 34 (qs <= 9).
// hv + 16: every wave runs kt = Kh / 16 full k-tiles and its Kh mod 16 <= 4 remaining components (Kh = components per wave) as a
// lane-layout TAIL instead of a k-tile of their own (entropy_mfma.h, TL = values per lane): one value for up to 4 components
// (K = 17..20, 33..36, 49..52 on one wave, 66..72 and 98..104 on two, 130..144 and 194..208 on four), two for 5..8 where that
// kernel keeps its registers (tail8_ok below).  VBMC_ENT_TAIL=0 keeps the padded k-tile (A/B runs; read once per process);
// the block-sparse mode (cutoff > 0) always does.
static bool mfma_entropy_fits(int D, int K, double cutoff, const LaunchSwitches& sw, int* qs_out, int* kt_out, int* hv_out) {
  const int qs = (D + 2 + 3) / 4;
  int hv = K <= 64 ? ent_hv_small(qs, K) : (K <= 128 ? ent_hv_mid(qs, K) : (K <= 256 ? 4 : 8));   // (round 5: eight waves for 256 < K <= 512, full k-tiles only)
  if (K > 64 && K <= 128 && (sw.ent_hv == 2 || sw.ent_hv == 4)) hv = sw.ent_hv;
  if (K > 32 && K <= 64 && (sw.ent_hv == 1 || sw.ent_hv == 2)) hv = sw.ent_hv;
  int kt = (((K + hv - 1) / hv) + 15) / 16;
  static const bool tail_on = [] { const char* e = getenv("VBMC_ENT_TAIL"); return !(e && !strcmp(e, "0")); }();
  {
    const int Kh = (K + hv - 1) / hv;      // components of the first waves (the last one may hold fewer: its tail lanes idle)
    static const int tail_max = [] { const char* e = getenv("VBMC_ENT_TAIL"); return e ? atoi(e) : 2; }();   // 0 / 1 / 2 values per lane at most (A/B runs)
    const int tl = (Kh % 16 + 3) / 4;         // tail values per lane that would be needed: 1 for 1..4 components, 2 for 5..8
    // two values per lane pay except where that kernel runs out of registers (tools/tail_sweep.py: 57 shapes x tail limit 0 / 1 / 2)
    const int ktf = Kh / 16, rem = Kh % 16;
    const bool tail8_ok = ktf == 1 || (hv == 1 && ktf == 2 && (qs >= 5 || rem <= 6)) || (hv == 1 && ktf == 3 && qs <= 4) ||
                          (hv > 1 && ktf == 2) || (hv > 1 && ktf == 3 && qs >= 5);
    if (tail_on && hv != 8 && Kh > 16 && tl >= 1 && tl <= tail_max && (tl == 1 || (tl == 2 && tail8_ok)) && !(cutoff > 0.0) && !(hv > 1 && ktf < 2)) {
      kt = ktf;
      hv += 16 * tl;
    }
  }
  *qs_out = qs; *kt_out = kt; *hv_out = hv;
  return qs >= 1 && qs <= 9 && K >= 1 && K <= 512 && kt >= 1 && kt <= 4 && !(hv == 2 && kt < 2) && !(hv == 4 && kt < 2) && !(hv == 8 && kt < 3) && !(hv > 16 && kt > 3);
}

// The log-joint record buffer holds LJ_CO_SPLIT records per hyper-sample (elbo_plan sizes it, lj_co_nsplit splits the training set into
// it) for the narrow batches whose log joint may run as a role; from half a chip of (hyper-sample, restart) pairs on, one record each.
static bool lj_records_split(int S, int R, int Rp, int num_cu) { return (long long)S * std::min(R, Rp) < num_cu / 2; }

// Splits of the training set per cell group of the log-joint role: per-workgroup set-up (exp table, tau / log tau) against the length of the
// dependent loop over the training set.  Single chain at the headline shape (260 cell groups, 25 slabs of 16 points), us per Adam
// iteration: 1 split 46.6, 2: 41.1, 3: 41.2, 4: 43.0, 6: 45.4, 8: 52.2 (more workgroups than wave slots) -> about 640 role workgroups per restart
static int lj_co_nsplit(const LaunchShape& sh, int num_cu, bool use_lane) {
  const int K = sh.dm.K, S = sh.dm.S;
  const long long cells = (long long)((K + 3) / 4) * S;   // per restart: a restart's bits do not depend on the batch it is in
  const int slabs = (sh.dm.N + 15) / 16;
  int ns = (int)std::max<long long>(1, std::min<long long>(std::min(LJ_CO_SPLIT, slabs), (640 + cells / 2) / cells));
  // (round 5) a BATCH wide enough that the record buffer holds one record per hyper-sample: one role workgroup per
  // cell group -- the restarts supply the parallelism the splits supply to a single chain
  if (!lj_records_split(S, sh.dm.R, sh.Rp, num_cu)) ns = 1;
  if (use_lane) ns = 1;      // (the lane kernel's role walks the LDS-staged training set whole)
  return ns;
}

// Is this pass's SHAPE one where the expected log joint runs as a role of the MFMA entropy launch (entropy_mfma.h CO = true)?  The fork and
// the sharding (plan_launch) still decide whether it does; the chunk model, the two chunk classes and the walk go by the shape alone.
static bool lj_co_shape(const LaunchShape& sh, int num_cu, const LaunchSwitches& sw, const LaunchChoice& L) {
  const long long SR = (long long)sh.dm.S * sh.Rp;        // (plan_restarts: the undivided batch decides)
  // ... and only where the ENTROPY launch is small too (K R waves per sample chunk: a single chain has 50, a batch of restarts over one
  // hyper-sample -- or an entropy-only evaluation, whose surrogate is a one-point stand-in -- can fill the chip by itself and wants the
  // kernels built for occupancy, not these)
  const long long KR = (long long)sh.dm.K * (sh.Rp > sh.dm.R ? sh.Rp : (long long)sh.dm.R * sh.rstride);
  const double lim_sr = 0.5, lim_kr = 2.0;     // the two width limits in units of the chip's compute units (other values measured in round 5: profiles/r05_experiments.md section 8)
  return !sw.lj_co_off && sw.lj_kernel != LaunchSwitches::MFMA && sh.Mh > 0 && L.use_mfma && ent_mfma_role_inst(L.qs, L.hv & 15) && !(sh.cutoff > 0.0) && sh.compute_grad &&
         !sh.lj_records && SR < lim_sr * num_cu && (sh.Rp > sh.dm.R || SR * sh.rstride < lim_sr * num_cu) &&   // (the undivided batch's choice when the restarts are dealt over devices)
         KR < lim_kr * num_cu && sh.dm.N > 1 &&
         // (round 4) ... and small in WORK, not only in width: with many sample tiles per wave (Ns = 1e4 per component: 313 tiles per
         // (component, restart)) the role's workgroups delay an entropy launch that fills the chip by itself -- R = 4 at the headline
         // shape: 0.242 ms with the role, 0.221 without; equal at R = 2 -- while at the optimiser's own sample counts (Ns = 28..400)
         // the role wins by 13-24 % for R <= 4.  The bound: sixteen sample tiles per resident wave slot.
         KR * ((sh.Mh + 15) / 16) <= 16LL * 8 * num_cu;
}

// Every launch decision of one pass.  `sharded`: the pass is one rank's share of a sharded evaluation (vbmc_elbo_shard_*), enqueued with
// ShardSpec.mode != 0 -- it runs the separate log-joint kernel the unsharded evaluation of the full S would, on this stream.
// false: the one shape this library has no kernel for (eight-wave workgroups whose LDS exceeds a compute unit's); L.qs / kt / hv are set.
static bool plan_launch(const LaunchShape& sh, const LaunchDevice& dev, bool sharded, const LaunchSwitches& sw, LaunchChoice& L) {
  const int D = sh.dm.D, K = sh.dm.K, R = sh.dm.R, S = sh.dm.S, N = sh.dm.N, Mh = sh.Mh, num_cu = dev.num_cu;
  const bool mc = Mh > 0, grad = sh.compute_grad != 0;
  if (mc) {      // ---- the entropy kernel class
    L.use_mfma = mfma_entropy_fits(D, K, sh.cutoff, sw, &L.qs, &L.kt, &L.hv) && sw.ent_kernel != LaunchSwitches::VALU;   // "valu" (A/B testing); default: the MFMA kernel when it fits
    // small mixtures: the lane-per-sample kernel (entropy_lane.h).  VBMC_ENT_KERNEL=mfma keeps the matrix-core kernel there (A/B runs, tests)
    L.use_lane = lane_entropy_fits(D, K, sh.cutoff) && sw.ent_kernel != LaunchSwitches::VALU && sw.ent_kernel != LaunchSwitches::MFMA &&
                 ((long long)K * sh.Rp * ((Mh + 63) / 64) >= ENT_LANE_MIN_TILES || sw.ent_kernel == LaunchSwitches::LANE);
    if (L.use_lane) L.use_mfma = false;
  }
  L.ent_form = !mc ? VBMC_ENTFORM_LB : (L.use_lane ? VBMC_ENTFORM_LANE : (L.use_mfma ? VBMC_ENTFORM_MFMA : VBMC_ENTFORM_VALU));

  // ---- the expected log joint: on the auxiliary stream beside the entropy kernel (fork), as a role of the entropy launch, or a launch of
  // its own on the pass's stream.  A pass on a slot stream has no auxiliary stream: the pass on the other slot stream is what fills in around
  // its entropy kernel, and a log joint forked off there is the last to be let onto the chip (profiles/r04_experiments.md section 11)
  const bool lane_role_possible = L.use_lane && grad && !sh.lj_records && N > 1 && lane_role_fits(D, K, N, S);
  L.fork = !sharded && mc && (long long)S * R >= num_cu / 2 && !dev.prof_alone && !lane_role_possible && ctx_aux(dev.aux_of);   // a single chain: the fork / join events cost more than they hide
  const bool lj_force = sw.lj_kernel == LaunchSwitches::MFMA, lj_valu = sw.lj_kernel == LaunchSwitches::VALU;
  // (round 6) the lane-per-sample kernel of small mixtures carries the role at every batch width: a pass of that class is ONE chip-wide launch
  const bool co_lane = lane_role_possible && !sharded && !lj_force && !sw.lj_co_off && !lj_valu;
  // Small grids (a single chain, a handful of restarts): the VALU log joint runs as a ROLE of the entropy launch (single-wave
  // workgroups ahead of the entropy ones, entropy_mfma.h CO = true) -- two dependent-chain-bound kernels side by side instead of
  // one after the other, one launch less.  Its records are per (hyper-sample, split of the training set); the reduction over
  // hyper-samples adds the splits.  VBMC_LJ_CO=0 keeps the separate launch (A/B runs, tests).
  const bool co_shape = lj_co_shape(sh, num_cu, sw, L);
  const bool co = co_lane || (!sharded && !L.fork && co_shape);      // (the role takes precedence over the matrix-core kernel where its limits admit the batch)
  // value + gradient: moments on the matrix cores (k_logjoint_mfma); value only: the VALU kernel.  VBMC_LJ_KERNEL=valu / mfma forces one of them.
  // One workgroup per (hyper-sample, restart): needs enough of them to fill the chip, otherwise (a single chain) the finer-grained VALU
  // kernel has the lower latency
  // (round 4: from S R = one workgroup per compute unit on -- below, the finer-grained VALU kernel is the faster one: R = 8 at the headline
  // shape, 160 (hyper-sample, restart) workgroups: 56 us against 34 alone, the step 0.394 -> 0.360 ms; equal at R = 16, 142 against 174 us at R = 64)
  // (round 5) ... and enough WAVES in each: with K <= 16 a workgroup of the matrix-core kernel is a single wave walking the whole training
  // set, and the VALU kernel's four waves per cell group are faster until the batch is several chips wide (BASELINE configs[1], K = 10,
  // S R = 512: 28.3 us against 19.9)
  const long long SRp = (long long)S * sh.Rp;
  const bool lj_wide = K > 16 || SRp >= 4LL * num_cu;
  // (round 6: value-only passes too -- the sieve's 250 candidates -- through the kernel's GRAD = false form, once the batch is four chips wide)
  // feature rows / moment exchange in LDS: large K x D falls back to the VALU kernel
  const bool lj_mfma = !co && (grad || SRp >= 4LL * num_cu) && K <= 256 && (lj_force || (SRp >= num_cu && lj_wide)) && !lj_valu &&
                       LJ_MFMA_DYN_LDS(sh.dt, (K + 15) / 16) + LJ_MFMA_STATIC_LDS <= 64 * 1024;
  // VALU kernel: four waves per cell (training set split, lower latency) while the grid is small, one wave per cell (no
  // replicated per-wave setup) once there are enough cells to fill the chip several times over
  L.lj_split = N > 64 && (long long)((K + 3) / 4) * S * sh.Rp < 8LL * num_cu;
  L.lj_form = co ? (L.use_lane ? VBMC_LJFORM_ROLE_LANE : VBMC_LJFORM_ROLE_MFMA)
                 : (lj_mfma ? (grad ? VBMC_LJFORM_MFMA_GRAD : VBMC_LJFORM_MFMA_VALUE) : (L.lj_split ? VBMC_LJFORM_VALU_SPLIT : VBMC_LJFORM_VALU_WAVE));
  if (!mc) return true;

  // ---- chunks per (component, restart): minimise  ceil(waves / resident slots) * (setup + tiles per wave),
  // i.e. whole rounds of resident waves, with the per-wave setup worth ~1.5 tiles
  const int tile_sz = L.use_lane ? 64 : (L.use_mfma ? 16 : 32);          // base samples per tile
  const int ntile = (Mh + tile_sz - 1) / tile_sz;
  // resident waves: what the chosen instantiation really holds per compute unit (registers AND LDS; round 3 -- rounds 1-2 assumed two
  // waves per SIMD for every MFMA kernel, which under-filled the chip for the small kernels that hold three or four)
  int waves_per_cu = L.use_mfma ? 8 : 5;
  if (L.use_mfma) {
    EntArgs q{};
    q.D = D; q.K = K; q.cutoff = sh.cutoff; q.lj.rows = co_shape ? 1 : 0;    // (the role-carrying kernel's occupancy wherever the SHAPE admits the role)
    const int nb = dev.mfma_occupancy(L.qs, L.kt, L.hv, grad, q);
    if (nb > 0) waves_per_cu = nb * (L.hv & 15);
    // eight-wave workgroups (K > 256): the parameter block, the parked exponents of eight waves and the PV exchange can exceed the
    // 160 KB of a compute unit at large D -- then no workgroup fits and the shape is refused (the VALU kernel's LDS does not
    // hold K > 256 either)
    if (nb <= 0 && (L.hv & 15) == 8) return false;
    // wide operands (D >= 15): the kernels that COULD hold more than eight waves (one k-tile) do not gain from shorter chunks -- their
    // per-wave set-up grows with D (D = 20, K = 8: 0.27 -> 0.37 ms with twelve assumed) -- while the ones that hold fewer (LDS: seven)
    // are where the correction pays (D = 28, K = 40: 1.36 -> 1.10 ms): profiles/r03_shape_sweep.md
    if (L.qs >= 5 && waves_per_cu > 8) waves_per_cu = 8;
  }
  if (L.use_lane) {
    const int nb = dev.lane_occupancy(D, K, grad);
    waves_per_cu = ENT_LANE_WAVES_HOST * (nb > 0 ? nb : 2);
  }
  const long long slots = (long long)num_cu * waves_per_cu * sh.cw;
  const long long kr = (long long)K * sh.Rp * (L.use_mfma ? (L.hv & 15) : 1);   // waves per chunk index (hv + 16 TL: with a component tail); Rp: R, or the undivided batch's (plan_restarts)
  const double setup = L.use_lane ? 1.0 : 1.5;   // (lane kernel: a tile of 64 samples is ~1.5 us, the set-up about that)  measured: C = 7 (45 tiles per wave) beats C = 5 (63) by 1 % at the headline shape once the setup loads are batched
  double best = 1e300;
  int bestC = 1;
  for (int c = 1; c <= ntile; ++c) {
    const int tpc = (ntile + c - 1) / c;
    const int ceff = (ntile + tpc - 1) / tpc;
    const long long rounds = (kr * ceff + slots - 1) / slots;
    const double cost = (double)rounds * (setup + tpc);
    if (cost < best - 1e-9) { best = cost; bestC = ceff; }
    if (tpc == 1) break;
  }
  if (sw.chunks_set && sw.chunks >= 1 && sw.chunks <= ntile) bestC = sw.chunks;
  if (sw.debug_occ) fprintf(stderr, "chunks: D %d K %d R %d qs %d kt %d hv %d waves/CU %d slots %lld kr %lld ntile %d -> C %d\n", D, K, R, L.qs, L.kt, L.hv, waves_per_cu, slots, kr, ntile, bestC);
  L.tpc = (ntile + bestC - 1) / bestC;
  L.C = (ntile + L.tpc - 1) / L.tpc;
  // the chunking is this launch's own to choose: not another launch's (sharded, plan_restarts), not forced
  const bool own_chunks = sh.cw == 1 && !sharded && sh.plan_restarts == 0 && !sw.chunks_set;
  // Two chunk classes where the launch carries the log-joint role (one or two restarts at Ns = 1e4: ~2000 entropy waves + 500-1000 role
  // waves on 2048 slots -- the role's waves went first and a quarter of the entropy waves entered a role late): the role's workgroups go
  // on to a chunk of the entropy that is a role's length (~4 tiles: 18 us) shorter, every wave of the launch is resident from the
  // start and all leave together.
  if (co_shape && own_chunks) {
    const int role_per_r = ((K + 3) / 4) * S * lj_co_nsplit(sh, num_cu, false);
    const long long waves0 = slots - (long long)role_per_r * R;
    const int TROLE = 4;                                   // a role in tiles (role + its later set-up against 4.5 us per tile of a wave that shares its SIMD)
    const int c1 = (int)(waves0 / ((long long)K * R)), c2max = role_per_r / K;
    if (c1 >= 1 && c2max >= 1 && ntile > TROLE * c1 + c1 + c2max) {
      const int tpc2 = (ntile - TROLE * c1 + c1 + c2max - 1) / (c1 + c2max);
      const int tpc1 = (ntile - c2max * tpc2 + c1 - 1) / c1;
      const int rest = ntile - c1 * tpc1;
      if (tpc2 >= 1 && tpc1 > tpc2 && rest > 0) {
        L.co_c1 = c1; L.co_tpc2 = tpc2; L.co_c2 = (rest + tpc2 - 1) / tpc2;
        L.tpc = tpc1; L.C = L.co_c1 + L.co_c2;
        if (sw.debug_occ) fprintf(stderr, "two chunk classes: %d x %d tiles + %d x %d tiles (role workgroups per restart %d)\n", c1, tpc1, L.co_c2, tpc2, role_per_r);
      }
    }
  }
  // The walk (entropy_mfma.h): once the chunk grid would hand every wave slot two or more waves, ONE wave per slot walks its share of
  // all the (restart, component) pairs' tiles instead -- a set-up per (wave, pair) instead of per chunk.  The device-RNG gradient kernels of
  // single-wave workgroups at D <= 14, K <= 56 (the instantiations that take the loop without spilling); not where
  // the bits must be those of another launch shape (sharded evaluation, plan_restarts) or the shape is the log-joint role's (so a walking
  // launch never carries a role or a shard).
  // Not for the passes of a pipeline either (vbmc_elbo_submit): there the short kernels of the NEXT pass take the slots the chunk grid's
  // waves free as they finish, and the step is the sum of its kernels' work with no gap at all (2.19 ms at the headline shape) -- a launch
  // whose waves all end together leaves them nothing until it is over (2.24); a blocking call or an optimiser iteration has no next pass
  // to interleave (2.29 -> 2.25 ms).  VBMC_ENT_WALK=0: the chunk grid (A/B runs, tests).
  const long long total = (long long)K * R * ntile;
  if (L.use_mfma && ent_mfma_walk_inst(L.qs, L.kt, L.hv & 15) && sh.eps_mode == 0 && grad && !(sh.cutoff > 0.0) && own_chunks && !sh.pipelined && !sw.walk_off &&
      kr * L.C >= 2 * slots && total < (1LL << 31) && !co_shape) {
    L.walk_tpw = (int)((total + slots - 1) / slots);
    L.walk_nw = (int)((total + L.walk_tpw - 1) / L.walk_tpw);
    L.C = ent_walk_max_slots(ntile, L.walk_tpw);
    if (sw.debug_occ) fprintf(stderr, "walk: %d waves x %d tiles, %d record slots per pair\n", L.walk_nw, L.walk_tpw, L.C);
  }
  if (co) {      // ---- the role's geometry
    L.co_nsplit = lj_co_nsplit(sh, num_cu, L.use_lane);
    L.co_nwg = ((K + 3) / 4) * S * L.co_nsplit;
    // the lane kernel's role is dealt over the entropy waves themselves (entropy_lane.h): no rows of its own.  Matrix-core kernel: the grid's
    // x extent is the chunks (two chunk classes: the first class), the role's workgroups -- and as many more as the second class needs -- follow in rows
    const int gx = L.co_c2 > 0 ? L.co_c1 : L.C;
    L.co_rows = L.use_lane ? 0 : (std::max(L.co_nwg, L.co_c2 > 0 ? K * L.co_c2 : 0) + gx - 1) / gx;
  }
  return true;
}
