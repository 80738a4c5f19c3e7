// Device-side data layout of one bundle-adjustment problem (one rank's shard)
// and the launchers of the LM-iteration kernels.  See DESIGN.md §3 for the
// HBM layout and the per-kernel roofline arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "ba_lm.h"    // the scalar block's indices (enum Scalar) and the LM state machine
#include "ba_plan.h"  // which kernel variant each pass runs (ProblemPlan, SolvePlan)

namespace sfm {

// Per-observation Jacobian record written by the Jacobian pass (doubles):
//   [0..5]  J_X  (2 x 3, row-major)   d r / d X          (scaled)
//   [6..7]  r    (2)                   residual
//   [8..19] J_c  (2 x 6, row-major)   d r / d (rot, t)   (scaled)
constexpr int kJRec = 20;
constexpr int kJX = 0, kRes = 6, kJC = 8;
// Back-substitution pass A output per observation, at its point-major slot:
// u = M^T e (3) | pad.
constexpr int kEU = 4;
// Per-camera rotation data: R (9, row-major) and dR/dw_k (27, k-major).
constexpr int kCamR = 36;
// Per-camera reduction record: U (21, packed upper 6x6), b_c (6), pad.
constexpr int kUcam = 28;
// Per-camera record of the one-pass point-major back substitution
// (k_backsub_pm; built in LDS by cam_step_record):
// R 9 | t 3 | K 5 | omega 3 | tau 3 | first-order flag | R_new 9 | t_new 3 |
// pad 2.  An even count: every record is 16-B aligned and is read with
// 16-byte loads (ds_read_b128, 256 B/clk; the 8-byte pairs an odd stride
// leaves run at half that).  Entries 0..23 are the first observation loop's,
// 12..17 and 24..35 the second's.
constexpr int kCamPM = 38;  // (kCamPMMax of them fit the 160-KB LDS: ba_plan.h)
constexpr int kCamPMFlag = 23, kCamPMNew = 24;
static_assert(kCamPM % 2 == 0 && kCamPMNew % 2 == 0, "16-byte reads of a record");
static_assert(kCamPM * int(sizeof(double)) == kCamPMBytes, "ba_plan.h sizes kCamPMMax by this record");
// Per-point record: V (6 packed lower), b_p (3), pad | L (6), z (3), pad.
constexpr int kPtV = 10;
constexpr int kPtL = 10;
// Per-point Schur record (k_schur_pts): X (3), Jacobi scale (3), L (6), 1/l_ii (3), pad: 128 B.
constexpr int kPtS = 16;
// Per-point record of k_schur_pairs_rot_pw: X (3), G_p = diag(s_p) L_p^-T (G00 G01 G02 G11 G12 G22), pad: 128 B.
constexpr int kPtG = 16;
// Per-camera record of k_schur_pairs_rot_pw's staging (one side of a block in LDS; camS):
// R 9 | t 3 | fx sk fy | first-order flag | J 9 (row-major) | Jacobi scale 6 | pad.
constexpr int kCamSR = 32;
// LDS bank rule of a 16-byte read (ds_read_b128): a wave's
// read is served in four 16-lane groups, {0-3, 12-15, 20-27} and {4-11,
// 16-19, 28-31} of each half, one LDS cycle per group when every distinct
// address of the group lies in a 16-B slot of its own of the 256-B bank row
// (equal addresses broadcast).  The degree returned is the largest number of
// distinct addresses of one group that share a slot, over the four groups,
// when lane l reads at (l / lanes_per_rec) * stride_doubles doubles plus an
// offset common to the wave: 1 = full rate, n = n LDS cycles per group.
constexpr int lds_b128_conflict_degree(int lanes_per_rec, int stride_doubles) {
  const int first[2][3] = {{0, 12, 20}, {4, 16, 28}}, count[2][3] = {{4, 4, 8}, {8, 4, 4}};
  int worst = 0;
  for (int half = 0; half < 2; ++half)
    for (int grp = 0; grp < 2; ++grp) {
      int rec_of[16] = {}, n = 0;  // the group's distinct records
      for (int run = 0; run < 3; ++run)
        for (int i = 0; i < count[grp][run]; ++i) {
          const int rec = (32 * half + first[grp][run] + i) / lanes_per_rec;
          bool seen = false;
          for (int j = 0; j < n; ++j) seen = seen || rec_of[j] == rec;
          if (!seen) rec_of[n++] = rec;
        }
      for (int a = 0; a < n; ++a) {
        int same = 0;
        for (int b = 0; b < n; ++b)
          same += (rec_of[a] * stride_doubles / 2) % 16 == (rec_of[b] * stride_doubles / 2) % 16 ? 1 : 0;
        worst = same > worst ? same : worst;
      }
    }
  return worst;
}
// Stride (doubles) of a block's two staged records, side by side, in
// k_schur_pairs_rot_pw's LDS image: 2 kCamSR + 2, so the blocks a lane group
// reads together sit 16 B apart mod 256 B.  (At 2 kCamSR = 512 B they are 4
// deep on the same banks with 8 lanes per block.)  camS in memory keeps kCamSR.
constexpr int kCamSRP = 2 * kCamSR + 2;
static_assert(kCamSRP % 2 == 0 && kCamSR % 2 == 0, "16-byte reads of both sides' records stay aligned");
static_assert(lds_b128_conflict_degree(8, kCamSRP) == 1 && lds_b128_conflict_degree(16, kCamSRP) == 1 &&
                  lds_b128_conflict_degree(32, kCamSRP) == 1 && lds_b128_conflict_degree(64, kCamSRP) == 1,
              "k_schur_pairs_rot_pw's record reads are conflict-free at every kSub");
static_assert(lds_b128_conflict_degree(8, 2 * kCamSR) == 4, "(the rule, on the unpadded stride)");
// Cholesky tile size.
constexpr int kNB = 64;
// Threads per workgroup of the observation / point kernels.
constexpr int kThreads = 256;
// k_backsolve's "not yet produced" value of a y entry (both halves: a
// signalling NaN, which arithmetic never yields)
constexpr uint32_t kYSentinelWord = 0x7FF4DEADu;
constexpr uint64_t kYSentinel = (uint64_t(kYSentinelWord) << 32) | kYSentinelWord;

// Batched scalar reductions (k_reduce_batch): job i reduces partial slot
// `slot` over `nb` blocks (op 0 sum, 1 max) into scal[dst].
struct ReduceJob {
  int slot, nb, op, dst;
};
struct ReduceBatch {
  ReduceJob job[8];
  int n = 0;
  void add(int slot, int nb, int op, int dst) { job[n++] = ReduceJob{slot, nb, op, dst}; }
};

struct DevProblem {
  ProblemPlan plan;          // set_problem's decisions (ba_plan.h); the arrays below exist as it says
  int32_t C = 0, P = 0;      // cameras (global), points (this shard)
  int64_t N = 0;             // observations (this shard)
  // structure (point-major observation order; within a point by camera,
  // then by the caller's order) -- built on the device by set_problem
  int32_t* pt_off = nullptr;   // [P+1]
  int32_t* order = nullptr;    // [N] caller's observation index of point-major q
  int64_t N_pad = 0;           // camera-major positions incl. per-camera padding to 64
  int32_t* cam_obs = nullptr;  // [N_pad] point-major observation id at camera-major position (-1: padding)
  int32_t* cam_rng = nullptr;  // [C][2] camera c's records: positions [begin, end)
  int32_t* cm_p = nullptr;     // [N_pad] point index at camera-major position i
  int4* jchunks = nullptr;     // [n_jchunks] (camera, first position, count, 0): k_jacobian work units
  int32_t n_jchunks = 0;
  int32_t xcd_slice_max = 0;   // chunks of the largest of the 8 point slices (host copy)
  int32_t* jgrp = nullptr;     // [9] chunk-table offsets of the 8 point slices (one per XCD)
  double* uv_cm = nullptr;     // [N_pad][2] uv in camera-major order
  int32_t* pos = nullptr;      // [N] camera-major position of point-major observation q
  double* Kc = nullptr;        // [C][5] fx skew cx fy cy
  // parameters (current and candidate)
  double* cam = nullptr;      // [C][6] rot(3) t(3)
  double* cam_new = nullptr;  // [C][6]
  double* X = nullptr;        // [P][3]
  double* X_new = nullptr;    // [P][3]
  double* cam0 = nullptr;     // [C][6] initial (reset)
  double* X0 = nullptr;       // [P][3]
  // Jacobi scaling and LM diagonal
  double* scale_c = nullptr;  // [C][6]
  double* scale_p = nullptr;  // [P][3]
  double* diag_c = nullptr;   // [C][6]
  double* diag_p = nullptr;   // [P][3]
  // per-iteration work arrays
  double* camR = nullptr;     // [C][36]
  double* camRn = nullptr;    // [C][12] candidate R (9) + t (3)
  double* jrec = nullptr;     // [N_pad][20] at camera-major position (J_X 6 | r 2 | J_c 12): evaluate API only,
                              // allocated on first use (the solve writes no records)
  double* eu = nullptr;       // [N_pad][kEU] back substitution pass A output, at camera-major positions
  double* ypt = nullptr;      // [P][3] point steps y_p (scaled space)
  int32_t* wcam = nullptr;    // [N_pad / 64] camera of each camera-major wavefront (runs padded to 64)
  double* ptV = nullptr;      // [P][10]
  double* ptL = nullptr;      // [P][10]
  double* Ucam = nullptr;     // [C][28]
  // reduced camera system: column-major lower (== row-major upper), ld x ld,
  // n = 6C unknowns, row n holds the reduced right-hand side (augmented).
  int32_t n = 0, ld = 0, nblk = 0;
  double* S = nullptr;
  double* Spack = nullptr;    // [n(n+1)/2 + n] packed upper triangle + rhs (cross-rank all-reduce)
  double* invL = nullptr;     // [nblk][64][64] inverses of the diagonal tiles
  double* ysol = nullptr;     // [ld] solution of S y = rhs (camera part)
  int32_t* fail = nullptr;    // [1] 1: Cholesky pivot not positive; 2: back-substitution hand-off timeout;
                              //     4: Cholesky tile hand-off timeout
  int32_t* flags = nullptr;   // [nblk] back-substitution hand-off flags (epoch-stamped)
  int32_t* cflags = nullptr;  // [2][nblk][nblk] fused Cholesky: final (F) and partial (P) tile flags
  unsigned long long* cticket = nullptr;  // [5] fused Cholesky tile ticket, its walker-role ticket, the back
                                          // substitution's row ticket (all monotone across launches); a
                                          // distributed factor panel's two (zeroed per panel)
  int32_t n_cu = 0;           // compute units (co-residency bound of the persistent grids)
  // LM diagonal clamp of the running solve (sfm_ba_options min/max_lm_diagonal)
  double min_diag = 1e-6, max_diag = 1e32;

  // Schur (k_schur_pts): every upper-triangle camera block (c1, c2), c1 <=
  // c2, in row-major order, the CSR offsets of its pair list and, per pair
  // (o1, o2) of a common point, that point; F is recomputed per pair from the
  // point and the two wave-uniform cameras
  int64_t n_blk = 0, n_pairs = 0;
  int2* blk = nullptr;        // [n_blk]
  int32_t* seg = nullptr;     // [n_blk + 1]
  int32_t* bpts = nullptr;    // [n_pairs]
  int32_t* bperm = nullptr;   // [n_bslots] k_schur_pts work order (XCD-aware row groups; -1: empty slot;
                              // nullptr: plain block order, without plan.xcd_block_order)
  int64_t n_bslots = 0;
  int4* srec = nullptr;       // [n_bslots] with bperm: slot k's {c1, c2, seg[b], seg[b + 1]}, b = bperm[k]; c1 = -1:
                              // empty slot (k_schur_pairs_rot_pw reads these in place of bperm -> blk -> seg)
  double* camS = nullptr;     // [C][kCamSR] with ptG: each camera's staged record (k_cam_stage_rot, once per pass)
  double* ptS = nullptr;      // [P][kPtS] X 3, scale 3, l10 l20 l21, 1/l_ii 3, z 3, pad
  double* ptG = nullptr;      // [P][16] X 3, G_p = diag(s_p) L_p^-T (6, upper), pad: k_schur_pairs_rot_pw's record
                              // (plan.large_system; nullptr: k_schur_pts and ptS alone)
  // per-wave diagonal-block / rhs partials from k_obs_prep_rc ([N_pad/64][27])
  double* dpart = nullptr;
  // per-chunk U_c / b_c partials from k_jacobian ([N_pad/64][27])
  double* jpart = nullptr;
  // point-major uv and camera index (k_point_eval_rc)
  double* uv_pm = nullptr;     // [N][2]
  int32_t* cam_pm = nullptr;   // [N]
  // the same stream wave-major, for the lane-per-point passes (k_point_eval_*,
  // k_backsub_pm): wave w = points 64 w .. 64 w + 63 holds m_w = its largest
  // view count slots, slot k of lane l at (woff[w] + k) * 64 + l, so a wave's
  // loads of one step are lane-contiguous.  With plan.wave_major; nullptr
  // otherwise (the passes read uv_pm / cam_pm)
  int32_t* woff = nullptr;     // [ceil(P / 64) + 1] exclusive sum of m_w
  double* uv_wm = nullptr;     // [64 woff[last]][2]
  int32_t* cam_wm = nullptr;   // [64 woff[last]] past a point's count: its last camera (0: none)
  // reductions
  double* partials = nullptr; // scratch [kNumPartialSlots][max_blocks]
  int32_t max_blocks = 0;
  double* scal = nullptr;     // [kNumScalars]
  double* scal_host = nullptr;  // pinned host mirror
  // device-driven LM loop (sfm_ba_solve_resident on an unsharded problem):
  // the gate of the phase being enqueued (kernels return at once when
  // *gate == 0) and the trust-region radius the kernels read; both nullptr
  // on the host-driven path
  const int32_t* gate = nullptr;
  const double* radius_dev = nullptr;
};

// Partial-sum slots (each max_blocks doubles).
enum PartialSlot {
  kPCost = 0, kPXNormCam, kPXNormPt, kPGradCam, kPGradPt, kPModel, kPNewCost, kPStepPt, kPStepCam, kPBad,
  kPBadCam, kPBadBack, kPModelPt,
  kNumPartialSlots
};

// ---- launchers (ba_kernels.hip) ----
// Which kernel a launcher starts is its variant argument's or the problem
// plan's say (ba_plan.h holds the conditions, once); a size of zero launches
// nothing.
void launch_cam_prep(const DevProblem& d, double* cam, bool count_norm, hipStream_t s);
// the device LM loop's accept folded in: cam_new -> cam, X_new -> X (grid >= the copy's workgroups)
void launch_cam_prep_accept(const DevProblem& d, bool count_norm, int grid, hipStream_t s);
// write_records: also store the 160-B records (evaluate API, bench roofline)
void launch_jacobian(const DevProblem& d, bool scaled, hipStream_t s, bool write_records = false);
void launch_cam_reduce(const DevProblem& d, hipStream_t s);
// mode 0: unscaled pass -> compute scale_c from colnorms; mode 1: diag (if !reuse) + gradient
void launch_cam_finalize(const DevProblem& d, int mode, bool reuse_diag, bool count_grad, hipStream_t s);
// launch_cam_reduce + launch_cam_finalize (reuse_diag false) in one launch
// (unsharded: no U_c all-reduce between them); gradient partials per camera
void launch_cam_sum_finalize(const DevProblem& d, int mode, bool count_grad, hipStream_t s);
// mode 0: unscaled pass -> scale_p; mode 1: V, b, diag (if !reuse), gradient, x-norm
// factor (mode 1): the pass also does launch_point_factor's work for the coming step's radius
void launch_point_eval(const DevProblem& d, PointPass v, int mode, bool reuse_diag, hipStream_t s,
                       bool factor = false, double radius = 0.0);
// launch_point_factor + launch_obs_prep
void launch_point_prep(const DevProblem& d, double radius, hipStream_t s);
// the per-wave diagonal-block / rhs partials (k_obs_prep_rc; reads the point records)
void launch_obs_prep(const DevProblem& d, hipStream_t s);
void launch_point_factor(const DevProblem& d, double radius, hipStream_t s);
// the diagonal blocks + rhs and the pair pass (WgBlocks: in one launch)
void launch_schur(const DevProblem& d, PairPass v, double radius, bool add_diag, hipStream_t s);
// its two parts: the diagonal blocks + rhs (k_schur_diag_sum) and the
// off-diagonal blocks
void launch_schur_diag(const DevProblem& d, double radius, bool add_diag, hipStream_t s);
// cams_staged: camS already holds the cameras' records (launch_cam_sum_diag)
void launch_schur_offdiag(const DevProblem& d, PairPass v, hipStream_t s, bool cams_staged = false);
// launch_cam_sum_finalize (mode 1, with the gradient partials) and
// launch_schur_diag in one launch (after launch_obs_prep, in the evaluation);
// stage_cams: and k_cam_stage_rot's records (SolvePlan::stage_cams)
void launch_cam_sum_diag(const DevProblem& d, double radius, bool add_diag, hipStream_t s, bool stage_cams = false);
// the scaled launch_jacobian and launch_obs_prep in one camera-major pass
// (k_jac_obs_prep; after the point pass that wrote ptS)
void launch_jac_obs_prep(const DevProblem& d, hipStream_t s);
void launch_pad_init(const DevProblem& d, hipStream_t s);
void launch_pack_upper(const DevProblem& d, bool unpack, hipStream_t s);
// dst = scale * src unless *gate == 0 (gate may be nullptr)
void launch_gated_copy(const double* src, double* dst, int64_t n, double scale, const int32_t* gate, hipStream_t s);
// (not with Backsub::OnePass: k_backsub_pm takes the camera step itself)
void launch_cam_update(const DevProblem& d, bool count_norm, hipStream_t s);
// CamSums::InPointPass: the point pass and the camera sums + finalisation
// (k_cam_sum_finalize's work) in one launch
void launch_point_eval_with_cams(const DevProblem& d, int mode, bool count_grad, hipStream_t s);
// OnePass takes the camera step too (launch_cam_update's work, count_norm as
// there: no launch_cam_update before it)
void launch_point_backsub(const DevProblem& d, Backsub v, hipStream_t s, bool cams_var = true, bool pts_var = true,
                          bool count_norm = false);
// grids of the XCD-ordered observation passes and of the back substitution's point pass (ba_plan.h)
inline int obs_xcd_blocks(const DevProblem& d) { return obs_xcd_blocks(d.N_pad, d.xcd_slice_max); }
inline int pt_xcd_blocks(const DevProblem& d) { return pt_xcd_blocks(d.P); }
void launch_cam_solve(const DevProblem& d, double radius, hipStream_t s);
// sum (op 0) or max (op 1) of `nb` partials in slot into scal[dst]
void launch_reduce(const DevProblem& d, int slot, int nb, int op, int dst, hipStream_t s);
void launch_reduce_batch(const DevProblem& d, const ReduceBatch& b, bool copy_fail, hipStream_t s);

// ---- dense Cholesky (chol_kernels.hip) ----
// cam_step >= 0: a small system's one-workgroup factor also takes the
// camera step (k_cam_update; cam_step > 0: with its step-length partial);
// returns whether it did
bool launch_cholesky(const DevProblem& d, int epoch, hipStream_t s, bool clear_fail = true, int cam_step = -1);
// W_k granules back to the sentinel (k_schur_diag_sum does this in the solve)
// sentinel_set: y already holds kYSentinel (k_pad_init wrote it)
void launch_backsolve(const DevProblem& d, int epoch, hipStream_t s, bool sentinel_set = false);

// ---- distributed factor: 1-D block-cyclic column panels of pt tiles
// (panel J on rank J % nranks; chol_kernels.hip) ----
// panel k of the trailing matrix factored in place (L, W_k) by its owner
int launch_cholesky_panel(const DevProblem& d, int k, int pt, int epoch, hipStream_t s);
// this rank's panels j in [j0, j1] (j > k) updated with panel k's L
void launch_panel_update(const DevProblem& d, int k, int j0, int j1, int pt, int nranks, int rank, hipStream_t s);
int panel_update_tiles(int nblk, int pt, int j0, int j1, int nranks, int rank);
// panel rectangles (columns col0..col1-1, rows c0_J..n) and buf at off[J]
// (device array, < 0: skipped; nullptr: every panel at off1); mode 0 packs
// S into buf, 1 unpacks buf into S, 2 adds buf into S
constexpr int kPanelPack = 0, kPanelUnpack = 1, kPanelAdd = 2;
void launch_panel_copy(const DevProblem& d, int mode, int pt, int col0, int col1, const int64_t* off, int64_t off1,
                       double* buf, hipStream_t s);
// the failure flag into (put) or OR-ed from a broadcast buffer's slot
void launch_fail_slot(const DevProblem& d, bool put, double* slot, hipStream_t s);
// a diagonally dominant augmented system (timing of the distributed factor)
void launch_spd_fill(double* A, int ld, int n, unsigned seed, hipStream_t s);

}  // namespace sfm
