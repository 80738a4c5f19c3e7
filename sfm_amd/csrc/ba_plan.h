// Which kernel variant every pass of the bundle adjuster runs, decided once on
// the host, as plain C++ (no HIP):
//
//   SolveKnobs    the SFM_* switches that select a path or a grid, parsed in
//                 one function (read_knobs) at the two times they always were:
//                 the problem's half in sfm_ba_set_problem, the solve's half at
//                 the start of each sfm_ba_solve_resident
//   ProblemPlan   what set_problem decides from the problem's shape and the
//                 knobs (plan_problem); stored with the problem
//                 (DevProblem::plan).  set_problem allocates what the plan
//                 asks for
//   SolvePlan     what one solve adds from its mode, its collectives and the
//                 knobs (plan_solve): per pass an enum naming the kernels it
//                 stands for, and the reduction batches' block counts.  The
//                 drivers and the launchers (ba_solver.hip, ba_kernels.hip)
//                 branch on it and decide nothing themselves
//
// Run-time state (the handle's prep_fresh, cams_staged, accept_grid) is not
// part of a plan.  Like ba_host_layout.h and ba_lm.h this header is compiled
// into the library and exercised by the CPU sanitizer program
// (tests/asan/asan_main.cpp); DESIGN.md's table "which kernel runs when" and
// the Python restatements of the tests (tests/irregular_cases.py) follow it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "ba_host_layout.h"
#include "../../include/sfm_amd.h"

namespace sfm {

// cameras whose records (kCamPM doubles each) fit the 160-KB LDS of k_backsub_pm
constexpr int kCamPMMax = 512;
constexpr int kCamPMBytes = 304;  // one record (kCamPM doubles, ba_device.h)
static_assert(kCamPMMax * kCamPMBytes + 128 <= 160 * 1024, "k_backsub_pm: the records and its reduction scratch in one CU's LDS");
// sizes up to which the deciding workgroup also makes the accepted step current (AcceptFold)
constexpr int kAcceptFoldMaxCams = 256;
constexpr int64_t kAcceptFoldMaxX = 3 * 8192;

// ---- the switches ----

inline const char* env_get(const char* name) { return std::getenv(name); }
inline bool env_flag(const char* name) {
  const char* v = env_get(name);
  return v && v[0] == '1';
}

struct SolveKnobs {
  // the problem's (sfm_ba_set_problem)
  bool small_setup = true;    // SFM_SMALL_SETUP    0: the sorted layout path for keyframe-sized problems too
  bool pm_wave_major = true;  // SFM_PM_WAVE_MAJOR  0: no wave-major copy of the point-major stream
  int schur_pts_sub = 0;      // SFM_SCHUR_PTS_SUB  8 / 32 / 64 (anything else: 16) lanes per block; 0: by pair count
  int schur_wg = -1;          // SFM_SCHUR_WG       1 / other: a workgroup per block forced on / off; -1: by shape
  int schur_wgs = 0;          // SFM_SCHUR_WGS      the persistent pair pass's grid, up to a multiple of 8; 0: by CUs
  bool force_pack = false;    // SFM_FORCE_PACK     1: the packed all-reduce path on one rank
  int jac_wg_per_xcd = 0;     // SFM_JAC_WG_PER_XCD > 0: workgroups per XCD of the solve's Jacobian pass
  // the solve's (sfm_ba_solve_resident)
  bool eval_split = false;      // SFM_EVAL_SPLIT     1: the evaluation's two camera-major passes apart
  bool pe_groups1 = false;      // SFM_PE_GROUPS1     1: the 256-thread point pass at 64 < C <= 512
  bool host_lm = false;         // SFM_HOST_LM        1: the host drives the loop
  bool lm_unfused = false;      // SFM_LM_UNFUSED     1: k_lm_* launches instead of k_reduce_batch_lm's tail
  bool no_accept_fold = false;  // SFM_NO_ACCEPT_FOLD 1: the accept copy stays in the evaluation's k_cam_prep
  int lm_batch = 0;             // SFM_LM_BATCH       iterations per batch, 1..64; 0: 3, then 2
};

enum KnobTime { kKnobsProblem = 1, kKnobsSolve = 2 };
using EnvGet = const char* (*)(const char*);

// Each switch accepts exactly what its site always did: "not 0" and "is 1"
// are different tests, and the numbers clamp differently.
inline void read_knobs(SolveKnobs* k, int when, EnvGet get = env_get) {
  auto not0 = [&](const char* n) { const char* v = get(n); return !(v && v[0] == '0'); };
  auto is1 = [&](const char* n) { const char* v = get(n); return v && v[0] == '1'; };
  if (when & kKnobsProblem) {
    k->small_setup = not0("SFM_SMALL_SETUP");
    k->pm_wave_major = not0("SFM_PM_WAVE_MAJOR");
    k->schur_pts_sub = hostlayout::schur_pts_sub_forced(get("SFM_SCHUR_PTS_SUB"));
    k->schur_wg = hostlayout::schur_wg_forced(get("SFM_SCHUR_WG"));
    const char* v = get("SFM_SCHUR_WGS");
    k->schur_wgs = v ? std::min(1 << 16, std::max(0, std::atoi(v)) + 7) / 8 * 8 : 0;
    k->force_pack = is1("SFM_FORCE_PACK");
    v = get("SFM_JAC_WG_PER_XCD");
    k->jac_wg_per_xcd = v ? std::max(0, std::atoi(v)) : 0;
  }
  if (when & kKnobsSolve) {
    k->eval_split = is1("SFM_EVAL_SPLIT");
    k->pe_groups1 = is1("SFM_PE_GROUPS1");
    k->host_lm = is1("SFM_HOST_LM");
    k->lm_unfused = is1("SFM_LM_UNFUSED");
    k->no_accept_fold = is1("SFM_NO_ACCEPT_FOLD");
    const char* v = get("SFM_LM_BATCH");
    k->lm_batch = v ? std::max(1, std::min(64, std::atoi(v))) : 0;
  }
}

// ---- grids that are pure functions of the shape ----

inline int blocks_for(int64_t n, int threads) { return int((n + threads - 1) / threads); }
// the XCD-ordered observation passes (k_obs_prep_rc, k_backsub_a_rc, k_backsub_c):
// one workgroup per 4 chunks, a multiple of 8 (one point slice per XCD); one
// wave per chunk of the LARGEST slice (slices differ by ~5% at C3; a grid
// sized by the mean left the largest slice's excess chunks to a second round
// of waves: 45.6 -> 50.0 us for k_obs_prep_rc)
inline int obs_xcd_blocks(int64_t N_pad, int32_t xcd_slice_max) {
  const int64_t per = xcd_slice_max > 0 ? (int64_t(xcd_slice_max) + 3) / 4 : ((N_pad / 64 + 3) / 4 + 7) / 8;
  return int(8 * std::max<int64_t>(1, per));
}
// the XCD-ordered point pass of the back substitution (k_backsub_b): workgroup
// b serves point slice b % 8 in blocks of 256 points
inline int pt_xcd_blocks(int P) {
  const int64_t per_slice = (int64_t(P) + 7) / 8;
  return int(8 * std::max<int64_t>(1, (per_slice + 255) / 256));
}

// ---- the problem ----

struct ProblemShape {
  int C = 0, P = 0;
  int64_t N = 0, N_pad = 0;
  int n_jchunks = 0;         // 64-wide wavefront chunks of the camera runs
  bool host_counts = false;  // the host counted the observations (SetupPlan::host_counts)
  bool small_fits = false;   // ... and they fit the small path's bounds (hostlayout::small_setup_fits)
  // known only after the layouts (the small path's bound, or the sorted
  // path's round trip); < 0: not yet, and what follows from them is provisional
  int64_t n_pairs = -1;   // the Schur shape's pair count: the host's estimate where it has one, else the device's
  int64_t wm_slots = -1;  // 64-lane slots of the wave-major stream

  int64_t n_blk() const { return int64_t(C) * (C + 1) / 2; }        // upper-triangle camera blocks
};

struct ProblemPlan {
  bool small_setup = false;      // the layouts without radix sorts (keyframe-sized problems)
  bool wave_major = false;       // the lane-per-point passes read the wave-major stream (uv_wm, cam_wm, woff)
  int schur_pts_sub = 8;         // lanes per block of the Schur pair pass: 8, 16, 32 or 64
  bool schur_wg_blocks = false;  // ... one block per 4-wave workgroup (few blocks with long pair lists)
  bool large_system = false;     // n_blk > kSchurXcdMinBlocks: the rotated-point pair pass (ptG, camS exist)
  bool xcd_block_order = false;  // ... and the XCD-aware slot order on the sorted path (bperm, srec exist)
  bool pm_backsub = false;       // large, C <= kCamPMMax: the back substitution may run as k_backsub_pm's one pass
  bool force_pack = false;       // the packed all-reduce path on one rank (Spack exists)
  int schur_wgs = 0;             // the persistent pair pass's grid; 0: eight workgroups per CU
  int jac_blocks = 8;            // persistent grid of the solve's Jacobian pass (the cost partials' count)
  int jac_blocks_rec = 8;        // ... of the record-writing variant (evaluate API, bench roofline)
};

inline ProblemPlan plan_problem(const ProblemShape& sh, const SolveKnobs& k) {
  ProblemPlan p;
  // multiples of 8 (one point slice per XCD); the record-free pass of the
  // solve (no 160-B stores) prefers the larger grid: 256 workgroups per XCD,
  // 0.256 -> 0.223 ms per C3 solve
  const int per_xcd = (sh.n_jchunks / 8 + 3) / 4;
  p.jac_blocks_rec = 8 * std::max(1, std::min(per_xcd, 128));
  p.jac_blocks = 8 * std::max(1, std::min(per_xcd, k.jac_wg_per_xcd > 0 ? k.jac_wg_per_xcd : 256));
  p.small_setup = sh.host_counts && k.small_setup && sh.small_fits;
  // not on the small path: the copy's two launches cost a keyframe-sized
  // one-shot solve 0.02 ms of 0.49 (C1), and a stream of at most 1.3 MB gains
  // nothing measurable from it (profiles/pm_wave_major_ab.txt); nor when its
  // padding is above the cap
  p.wave_major = sh.N > 0 && sh.P > 0 && !p.small_setup && k.pm_wave_major &&
                 (sh.wm_slots < 0 || hostlayout::wave_major_fits(sh.wm_slots, sh.N, sh.P));
  const hostlayout::SchurShape ss =
      hostlayout::schur_shape(std::max<int64_t>(0, sh.n_pairs), sh.n_blk(), k.schur_pts_sub, k.schur_wg);
  p.schur_pts_sub = ss.pts_sub;
  p.schur_wg_blocks = ss.wg_blocks;
  p.large_system = sh.n_blk() > kSchurXcdMinBlocks;
  p.xcd_block_order = p.large_system && !p.small_setup;
  p.pm_backsub = p.large_system && sh.C <= kCamPMMax;
  p.force_pack = k.force_pack;
  p.schur_wgs = k.schur_wgs;
  return p;
}

// rows of the partial-sum scratch: every grid that writes per-block partials
inline int max_blocks(const ProblemShape& sh, const ProblemPlan& p, int32_t xcd_slice_max) {
  return std::max({1, sh.C, blocks_for(sh.N, 256), blocks_for(sh.P, 256), p.jac_blocks, p.jac_blocks_rec,
                   blocks_for(sh.N_pad, 256), obs_xcd_blocks(sh.N_pad, xcd_slice_max), pt_xcd_blocks(sh.P)});
}

// ---- one solve ----

// who runs ba_lm.h's transitions
enum class LmDriver {
  Host,                   // run_host_lm: a scalar readback per phase
  Device,                 // k_lm_init / k_lm_decide / k_lm_post, one launch each
  DeviceFused,            // the last workgroup of k_reduce_batch_lm
  DeviceFusedAcceptFold,  // ... which also makes an accepted candidate current
};
// the evaluation's camera sums U_c, b_c and their finalisation
enum class CamSums {
  None,                     // cameras constant: zeroed partials
  InPointPass,              // k_point_eval_lds<64> with CamFold
  SumFinalize,              // k_cam_sum_finalize
  ReduceAllreduceFinalize,  // k_cam_sum, the all-reduce of Ucam, k_cam_finalize
  SumDiag,                  // the step's prep folded: k_cam_sum_diag, after the point pass and the
                            // observation prep (the unscaled first pass: k_cam_sum_finalize)
};
// the evaluation's scaled camera-major pass
enum class CamPass {
  Jacobian,    // k_jacobian first (and k_obs_prep_rc after the point pass where the prep is folded)
  JacObsPrep,  // k_jac_obs_prep after the point pass
};
enum class PointPass {
  Lds64,     // k_point_eval_lds<64>
  Lds512x2,  // k_point_eval_lds<512, 2>: two 256-thread groups share one camera copy
  Lds512,    // k_point_eval_lds<512>
  Rc,        // k_point_eval_rc
};
// the Schur pair pass (the off-diagonal blocks)
enum class PairPass {
  WgBlocks,       // k_schur_pts<64, 4>: a workgroup per block, with the diagonal blocks (DiagFold)
  Pts,            // k_schur_pts<sub>
  RotPersistent,  // k_cam_stage_rot<sub> unless the evaluation staged the cameras, then k_schur_pairs_rot_pw<sub>
};
enum class Backsub {
  OnePass,    // k_backsub_pm, the camera step included
  ThreePass,  // k_cam_update, k_backsub_a_rc, k_backsub_b, k_backsub_c
};

struct SolveShape {
  int C = 0, P = 0;
  int64_t N_pad = 0;
  int32_t xcd_slice_max = 0;  // chunks of the largest of the 8 point slices
};

struct SolvePlan {
  int32_t mode = SFM_BA_STRUCT_AND_POSE;
  bool cams_var = true, pts_var = true;  // constant blocks: cameras in STRUCT_ONLY, points in POSE_ONLY
  bool sharded = false;
  LmDriver lm = LmDriver::Host;
  int lm_batch = 0;  // the device driver's fixed batch size; 0: 3, then 2
  // evaluation
  bool prep_folded = false;  // it also prepares the coming step: point factor, observation prep, diagonal blocks
  CamSums cam_sums = CamSums::None;
  CamPass cam_pass = CamPass::Jacobian;
  PointPass point_pass = PointPass::Lds64;  // (run while pts_var; its point factor folded in: prep_folded)
  bool stage_cams = false;                  // k_cam_sum_diag also leaves the cameras' staged records (camS)
  // step
  PairPass pair_pass = PairPass::Pts;
  bool cam_records_used = false;  // the pair pass reads camS
  bool dist_factor = false;       // the distributed factor's panel loop
  bool pack_allreduce = false;    // the packed upper triangle + rhs all-reduced before the factor
  Backsub backsub = Backsub::ThreePass;
  // block counts of the closing reductions
  int nb_cost = 1, nb_grad_cam = 1;  // evaluation: k_jacobian's grid; per camera, or per 256 cameras
  int nb_cam = 1, nb_pt = 1;         // per 256 cameras / points
  int nb_obs = 1, nb_back = 1;       // step: the observation passes' grid, the point pass's (OnePass: nb_pt)

  bool fused_lm() const { return lm == LmDriver::DeviceFused || lm == LmDriver::DeviceFusedAcceptFold; }
  bool accept_fold() const { return lm == LmDriver::DeviceFusedAcceptFold; }
};

// host_callbacks: a host collective is set (sfm_ba_set_host_comm /
// sfm_ba_set_host_collectives); dist_pt: the distributed factor's panel width
inline SolvePlan plan_solve(const ProblemPlan& pp, const SolveShape& sh, int32_t mode, bool sharded,
                            bool host_callbacks, int dist_pt, const SolveKnobs& k) {
  SolvePlan s;
  const int C = sh.C, P = sh.P;
  const bool both = mode == SFM_BA_STRUCT_AND_POSE;
  s.mode = mode;
  s.cams_var = mode != SFM_BA_STRUCT_ONLY;
  s.pts_var = mode != SFM_BA_POSE_ONLY;
  s.sharded = sharded;
  // the loop's decisions on the device unless a collective needs the host
  // between the phases (the host-callback hook; the distributed factor's
  // panel loop: at the sizes it is for, a host round trip per phase is noise).
  // Without a collective between a phase's reduction and the bookkeeping the
  // two are one launch
  s.dist_factor = sharded && dist_pt > 0;
  const bool host_lm = host_callbacks || s.dist_factor || k.host_lm;
  const bool fuse_lm = !host_lm && !sharded && !k.lm_unfused;
  const bool accept_fold =
      fuse_lm && C > 0 && C <= kAcceptFoldMaxCams && 3 * int64_t(P) <= kAcceptFoldMaxX && !k.no_accept_fold;
  s.lm = host_lm ? LmDriver::Host
                 : accept_fold ? LmDriver::DeviceFusedAcceptFold : fuse_lm ? LmDriver::DeviceFused : LmDriver::Device;
  s.lm_batch = k.lm_batch;
  // Unsharded STRUCT_AND_POSE beyond the small systems whose camera sums ride
  // in the point pass: the evaluation prepares the coming step.  A sharded
  // solve has a collective between the sums and their use and keeps the
  // stand-alone sequence, as do POSE_ONLY and STRUCT_ONLY
  s.prep_folded = both && !sharded && P > 0 && C > 64 && sh.N_pad > 0 && !pp.schur_wg_blocks;
  s.cam_pass = s.prep_folded && !k.eval_split ? CamPass::JacObsPrep : CamPass::Jacobian;
  const bool cams_in_point_pass = !sharded && s.cams_var && s.pts_var && P > 0 && C > 0 && C <= 64;
  s.cam_sums = cams_in_point_pass ? CamSums::InPointPass
               : s.prep_folded    ? CamSums::SumDiag
               : !s.cams_var      ? CamSums::None
               : sharded          ? CamSums::ReduceAllreduceFinalize
                                  : CamSums::SumFinalize;
  // camera constants from LDS while they fit (C3: 500 cameras, 68 KB)
  s.point_pass = C <= 64 ? PointPass::Lds64
                 : C <= 512 && !k.pe_groups1 ? PointPass::Lds512x2
                 : C <= 512 ? PointPass::Lds512 : PointPass::Rc;
  s.pair_pass = pp.schur_wg_blocks ? PairPass::WgBlocks : pp.large_system ? PairPass::RotPersistent : PairPass::Pts;
  s.cam_records_used = C > 0 && pp.large_system && pp.xcd_block_order && !pp.schur_wg_blocks;
  s.stage_cams = s.cam_pass == CamPass::JacObsPrep && s.cam_records_used;
  s.pack_allreduce = sharded || pp.force_pack;
  s.backsub = pp.pm_backsub && s.cams_var && s.pts_var && P > 0 && sh.N_pad > 0 ? Backsub::OnePass : Backsub::ThreePass;
  s.nb_pt = std::max(1, blocks_for(P, 256));
  s.nb_cam = std::max(1, blocks_for(C, 256));
  s.nb_cost = pp.jac_blocks;
  s.nb_grad_cam = s.cams_var && !sharded ? std::max(1, C) : s.nb_cam;
  // (k_backsub_pm: every partial per 256-point block)
  const bool one = s.backsub == Backsub::OnePass;
  s.nb_obs = one ? s.nb_pt : sh.N_pad ? obs_xcd_blocks(sh.N_pad, sh.xcd_slice_max) : 1;
  s.nb_back = one ? s.nb_pt : P ? pt_xcd_blocks(P) : 1;
  return s;
}

}  // namespace sfm
