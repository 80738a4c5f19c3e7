// Host side of sfm_ba_set_problem's layout, as plain C++ (no HIP): the
// keyframe-sized problems' checks and counts (k_validate's work done on the
// host), the camera runs and wavefront chunk table, the small path's XCD
// slice sizes and the bound of the camera-run blob staged for upload.
// Also the decisions set_problem takes before its first device call
// (plan_setup: which of the three regimes and four parameter routes a problem
// takes, and where its blobs lie in the pinned stage), the small path's size
// predicate and the Schur pass's shape.
// Kept apart from ba_problem.hip so that the CPU sanitizer build
// (tests/asan, `make asan`) runs exactly this code under ASan/UBSan.
//
// Reference: the observation / parameter-block layout is CSfM.cpp:310-341
// (one Ceres residual block per observation, CTracker.cpp:679-694); the
// checks are what the device validation (ba_setup.hip k_validate) reports.
#ifndef SFM_BA_HOST_LAYOUT_H_
#define SFM_BA_HOST_LAYOUT_H_

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace sfm {

// Transfers above this go straight from / to the caller's pageable memory:
// the runtime pipelines its own staging copies with the DMA, where ours
// would run them one after the other (C3 one-shot 7.4 -> 9.2 ms with the
// 48-MB observation upload staged).
constexpr size_t kStageMaxBytes = size_t(1) << 20;
// observations up to which set_problem checks and counts them on the host
constexpr int64_t kHostCheckMaxObs = 65536;
// and from which uv (16 B each) goes up from a worker thread beside the index
// layouts (4 MB: the thread's start-up is noise beside the copy)
constexpr int64_t kDeferredUvMinObs = 262144;
// Bounds of the layouts without radix sorts (ba_setup.hip small path): C <=
// 256, at most kSmallSetupMaxChunks chunks, short point segments.
constexpr int kSmallSetupMaxC = 256;
constexpr int kSmallSetupMaxChunks = 2048;
constexpr int kSmallSetupMaxPtObs = 64;
constexpr int64_t kSmallSetupMaxObs = 64 * 1024;  // (k_small_cm_compact: 64 steps of 1024)
// Reduced systems with more camera blocks than this take the XCD-aware
// k_schur_pts order (C3: 125k blocks); smaller ones the plain order.
constexpr int64_t kSchurXcdMinBlocks = 8192;

namespace hostlayout {

// byte offsets of a packed staging layout (256-B aligned pieces)
struct StageLayout {
  size_t bytes = 0;
  size_t add(size_t n) {
    const size_t o = bytes;
    bytes += (n + 255) & ~size_t(255);
    return o;
  }
};

// Bytes the camera-run blob (cam_rng | wcam | cam_off | chunks, and on the
// small path pt_off | the scatters' slot counters) can take, staged behind
// the still-in-flight input blob: 2 C + (npad / 64 + 1) + (C + 1) ints, 16 B
// per chunk (npad / 64 <= N / 64 + C chunks), P + 1 + P + C ints, padding.
inline size_t runs_blob_bound(int C, int64_t N, int P) {
  return 64 * (size_t(C) + 1) + 2 * size_t(N) + 8 * (size_t(P) + 1) + 4 * size_t(C) + 2048;
}

// How the parameter blob (Kc | cam | cam0 | X | X0) reaches the device.
//   None   no cameras and no points: nothing to upload
//   Early  host-counted problems: staged behind the camera-run blob and
//          uploaded before the layout launches (its host copies overlap them)
//   Side   above the stage's 1 MB: from the caller's pageable arrays on a
//          stream of its own beside the layout kernels
//   Late   staged after the layout round trip, which has freed the stage
enum class ParamRoute { None, Early, Side, Late };

// Everything set_problem decides before its first device call.
//
//   regime           observations        validation  uv upload
//   host counts      input blob <= 1 MB  host        staged with the indices
//   device checks    up to 262143        k_validate  in line, pageable
//   deferred uv      from 262144         k_validate  worker thread, side stream
//
// The pinned stage holds up to three regions at once, none synchronised
// against the next: the input blob [0, in_bytes), the camera-run blob
// [il_base, il_base + il_bound) and, on the Early route, the parameter blob
// [pl_base, pl_base + pl_bytes).
struct SetupPlan {
  bool host_counts = false;  // checks and counts on the host, riding in the staged input blob
  bool stage_in = false;     // the input blob goes through the pinned stage
  bool deferred_uv = false;  // uv from a worker thread beside the index layouts
  size_t o_uv = 0, o_cam = 0, o_pt = 0, o_pc = 0, in_bytes = 0;  // input blob (device, and the stage's image of it)
  size_t il_base = 0, il_bound = 0;                              // camera-run blob in the stage
  size_t o_K = 0, o_c = 0, o_c0 = 0, o_X = 0, o_X0 = 0, pl_bytes = 0;  // parameter blob
  size_t pl_base = 0;                                            // ... in the stage (Early)
  ParamRoute route = ParamRoute::None;
  size_t stage_bytes = 0;  // to reserve in the stage before the first upload
};

inline SetupPlan plan_setup(int64_t N, int C, int P, bool sync_uv) {
  SetupPlan p;
  // keyframe-sized problems: the checks and the camera / point counts on
  // the host, their point counts riding in the same upload -- no validation
  // launch and no round trip before the layout (C1: ~60 us of set_problem)
  const bool host_check = N <= kHostCheckMaxObs;
  StageLayout up;
  p.o_uv = up.add(sizeof(double) * 2 * size_t(N));
  p.o_cam = up.add(sizeof(int32_t) * size_t(N));
  p.o_pt = up.add(sizeof(int32_t) * size_t(N));
  p.o_pc = host_check ? up.add(sizeof(int32_t) * (size_t(P) + 1)) : 0;
  p.in_bytes = up.bytes;
  p.stage_in = p.in_bytes <= kStageMaxBytes;
  p.host_counts = host_check && p.stage_in;
  // large problems: uv uploaded beside the index layouts (SFM_SYNC_UV=1: in
  // line, as before round 6)
  p.deferred_uv = !p.stage_in && N >= kDeferredUvMinObs && !sync_uv;
  // (host counts: the camera-run blob is staged AFTER the input blob, which
  // is still in flight -- no synchronisation in between -- so the stage
  // holds both from the start: 2 C + chunks + ... ints, bounded)
  p.il_base = p.host_counts ? (p.in_bytes + 255) / 256 * 256 : 0;
  p.il_bound = p.host_counts ? runs_blob_bound(C, N, P) : 0;
  // intrinsics, the parameters and their reset copies: one blob, one DMA
  StageLayout pl;
  p.o_K = pl.add(sizeof(double) * 5 * size_t(C));
  p.o_c = pl.add(sizeof(double) * 6 * size_t(C));
  p.o_c0 = pl.add(sizeof(double) * 6 * size_t(C));
  p.o_X = pl.add(sizeof(double) * 3 * size_t(P));
  p.o_X0 = pl.add(sizeof(double) * 3 * size_t(P));
  p.pl_bytes = pl.bytes;
  p.pl_base = (p.il_base + p.il_bound + 255) / 256 * 256;
  if (!(C || P)) p.route = ParamRoute::None;
  else if (p.host_counts && p.pl_base + p.pl_bytes <= 4 * kStageMaxBytes) p.route = ParamRoute::Early;
  else if (p.pl_bytes > kStageMaxBytes) p.route = ParamRoute::Side;
  else p.route = ParamRoute::Late;
  p.stage_bytes = std::max({p.stage_in ? p.il_base + p.il_bound : 0,
                            p.route == ParamRoute::Early ? p.pl_base + p.pl_bytes : 0,
                            sizeof(int32_t) * (size_t(C) + 4)});  // (the validation readback: 4 + C counts)
  return p;
}

// The size part of the small path's predicate (the layouts without radix
// sorts; the caller adds that the host has the counts, and SFM_SMALL_SETUP):
// the segments fit ba_setup.hip's bounds, and C (C + 1) / 2 <=
// kSchurXcdMinBlocks, i.e. the plain k_schur_pts block order, as the sorted
// path takes for these sizes.
inline bool small_setup_fits(int64_t N, int C, int P, const int32_t* n_obs_of_cam, const int32_t* n_obs_of_pt) {
  if (!(N > 0 && N <= kSmallSetupMaxObs && C > 0 && C <= kSmallSetupMaxC &&
        int64_t(C) * (C + 1) / 2 <= kSchurXcdMinBlocks))
    return false;
  int64_t nch = 0;
  for (int c = 0; c < C; ++c) nch += (n_obs_of_cam[c] + 63) / 64;
  if (nch > kSmallSetupMaxChunks) return false;
  for (int p = 0; p < P; ++p)
    if (n_obs_of_pt[p] > kSmallSetupMaxPtObs) return false;
  return true;
}

// The wave-major copy of the point-major stream (DevProblem::uv_wm): wave w
// of 64 consecutive points takes as many 64-lane slots as its longest point
// has observations.  The copy is made only while its padded size 64 * slots
// stays within 1.5 N + 64 ceil(P / 64) entries (regular visibility: exactly
// N; one long track among short ones pads its whole wave).
inline bool wave_major_fits(int64_t slots, int64_t N, int P) {
  return 128 * slots <= 3 * N + 128 * ((int64_t(P) + 63) / 64);
}

// The Schur pass's shape from the mean pair count per camera block.  Lanes
// per block ~ a tenth of the mean, 8..64 (measured best: C3, 72 pairs per
// block -> 8; C1 / C2, ~460 -> 64; SFM_SCHUR_PTS_SUB forces 8 / 16 / 32 / 64).
// Few blocks with long lists (keyframe-sized: C1 210 blocks of ~460 pairs): a
// workgroup per block instead of a wave (SFM_SCHUR_WG=0/1 forces).  The
// overrides are the variables' values, nullptr when unset, or those values
// parsed (what ba_plan.h's SolveKnobs keeps): pts_sub_forced 0 and wg_forced
// -1 when unset.
struct SchurShape {
  int pts_sub = 8;
  bool wg_blocks = false;
};
inline int schur_pts_sub_forced(const char* v) {
  if (!v) return 0;
  const int n = std::atoi(v);
  return n == 64 ? 64 : n == 32 ? 32 : n == 8 ? 8 : 16;
}
inline int schur_wg_forced(const char* v) { return v ? (v[0] == '1' ? 1 : 0) : -1; }
inline SchurShape schur_shape(int64_t n_pairs, int64_t n_blk, int pts_sub_forced, int wg_forced) {
  SchurShape sh;
  const double avg = n_blk ? double(n_pairs) / double(n_blk) : 0.0;
  if (pts_sub_forced) {
    sh.pts_sub = pts_sub_forced;
  } else {
    while (sh.pts_sub < 64 && sh.pts_sub < avg / 10.0) sh.pts_sub *= 2;
  }
  sh.wg_blocks = sh.pts_sub == 64 && n_blk <= 4 * 256 && avg >= 256.0;
  if (wg_forced >= 0) sh.wg_blocks = wg_forced == 1 && sh.pts_sub == 64;
  return sh;
}
inline SchurShape schur_shape(int64_t n_pairs, int64_t n_blk, const char* pts_sub_env, const char* wg_env) {
  return schur_shape(n_pairs, n_blk, schur_pts_sub_forced(pts_sub_env), schur_wg_forced(wg_env));
}

// One 64-wide wavefront chunk of a camera's run (the int4 the device reads:
// camera, first camera-major position, count, the first observation's index
// in camera-major order).
struct Chunk {
  int32_t cam, pos, cnt, first;
};
static_assert(sizeof(Chunk) == 16, "Chunk must match the device's int4");

// The checks and counts of the observation arrays (k_validate's, on the host).
//   cam_cnt [C + 4]: [0..2] the first observation with a camera index out of
//     range / a point index out of range / a non-finite uv (INT32_MAX: none),
//     [3] = INT32_MAX, [4 + c] observations of camera c;
//   pc [P + 1]: observations of point p (pc[P] = 0);
//   cam_slice (want_slices): [C][8] observations of camera c in point slice s
//     (the 8 XCD slices of k_small_chunks' key: slice of p = floor(8 p / P));
//   pairs_est: sum over points of pc (pc - 1) / 2 -- every unordered pair of a
//     point's observations, i.e. the Schur pair total when no camera sees a
//     point twice (same-camera duplicates make it undercount; it is used for
//     the Schur pass's lane choice and, doubled, as the pair buffer's bound).
// Fast pass: the checks OR-ed without branches and the counts in four
// interleaved histograms (consecutive observations of one camera would
// otherwise chain every increment through a store-to-load dependency); only a
// problem with a bad observation takes the exact first-index pass.
inline void check_and_count(int64_t N, const double* obs_uv, const int32_t* cam_idx, const int32_t* pt_idx, int C,
                            int P, bool want_slices, int32_t* cam_cnt, int32_t* pc, std::vector<int32_t>* cam_slice,
                            int64_t* pairs_est) {
  int32_t first[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
  std::fill(cam_cnt, cam_cnt + size_t(C) + 4, 0);
  std::fill(pc, pc + size_t(P) + 1, 0);
  cam_slice->clear();
  *pairs_est = 0;
  const uint64_t* uvb = reinterpret_cast<const uint64_t*>(obs_uv);
  auto nonfinite = [](uint64_t b) { return uint32_t(((b >> 52) & 0x7ff) == 0x7ff); };
  uint32_t bad = 0;
  {
    std::vector<int32_t> cc4(4 * (size_t(C) + 1), 0), pc4(4 * (size_t(P) + 1), 0);
    want_slices = want_slices && P > 0;
    // slice s = floor(8 p / P) holds p >= ceil(s P / 8): seven comparisons
    uint32_t sb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 1; k < 8; ++k) sb[k] = uint32_t((int64_t(k) * P + 7) / 8);
    auto slice_of = [&](uint32_t p) {
      uint32_t v = 0;
      for (int k = 1; k < 8; ++k) v += uint32_t(p >= sb[k]);
      return v;
    };
    std::vector<int32_t> cs4(want_slices ? 4 * 8 * (size_t(C) + 1) : 0, 0);
    int64_t i = 0;
    for (; i + 4 <= N; i += 4) {
      for (int u = 0; u < 4; ++u) {
        const uint32_t c = uint32_t(cam_idx[i + u]), p = uint32_t(pt_idx[i + u]);
        const uint32_t b = uint32_t(c >= uint32_t(C)) | uint32_t(p >= uint32_t(P)) | nonfinite(uvb[2 * (i + u)]) |
                           nonfinite(uvb[2 * (i + u) + 1]);
        bad |= b;
        // (an out-of-range index lands in the spare slot C / P: the counts
        // are discarded with the error anyway)
        const uint32_t cc = c < uint32_t(C) ? c : uint32_t(C);
        ++cc4[u * (size_t(C) + 1) + cc];
        ++pc4[u * (size_t(P) + 1) + (p < uint32_t(P) ? p : uint32_t(P))];
        if (want_slices) ++cs4[(u * (size_t(C) + 1) + cc) * 8 + slice_of(p)];
      }
    }
    for (; i < N; ++i) {
      const uint32_t c = uint32_t(cam_idx[i]), p = uint32_t(pt_idx[i]);
      bad |= uint32_t(c >= uint32_t(C)) | uint32_t(p >= uint32_t(P)) | nonfinite(uvb[2 * i]) |
             nonfinite(uvb[2 * i + 1]);
      const uint32_t cc = c < uint32_t(C) ? c : uint32_t(C);
      ++cc4[cc];
      ++pc4[p < uint32_t(P) ? p : uint32_t(P)];
      if (want_slices) ++cs4[size_t(cc) * 8 + slice_of(p)];
    }
    if (want_slices) {
      cam_slice->assign(8 * size_t(C), 0);
      for (size_t e = 0; e < 8 * size_t(C); ++e)
        (*cam_slice)[e] = cs4[e] + cs4[8 * (size_t(C) + 1) + e] + cs4[16 * (size_t(C) + 1) + e] +
                          cs4[24 * (size_t(C) + 1) + e];
    }
    for (int c = 0; c < C; ++c)
      cam_cnt[4 + size_t(c)] =
          cc4[c] + cc4[(size_t(C) + 1) + c] + cc4[2 * (size_t(C) + 1) + c] + cc4[3 * (size_t(C) + 1) + c];
    for (int p = 0; p < P; ++p) {
      pc[p] = pc4[p] + pc4[(size_t(P) + 1) + p] + pc4[2 * (size_t(P) + 1) + p] + pc4[3 * (size_t(P) + 1) + p];
      *pairs_est += int64_t(pc[p]) * (pc[p] - 1) / 2;
    }
  }
  if (bad) {
    for (int64_t i = 0; i < N; ++i) {
      const int32_t c = cam_idx[i], p = pt_idx[i];
      const bool cok = c >= 0 && c < C, pok = p >= 0 && p < P;
      const bool uok = std::isfinite(obs_uv[2 * i]) && std::isfinite(obs_uv[2 * i + 1]);
      if (!cok && first[0] == INT32_MAX) first[0] = int32_t(i);
      if (!pok && first[1] == INT32_MAX) first[1] = int32_t(i);
      if (!uok && first[2] == INT32_MAX) first[2] = int32_t(i);
    }
  }
  cam_cnt[0] = first[0];
  cam_cnt[1] = first[1];
  cam_cnt[2] = first[2];
  cam_cnt[3] = INT32_MAX;
}

// Camera runs: camera-major, each camera's run padded to a whole number of
// 64-wide wavefront chunks; wcam[w] = the camera of chunk slot w; the chunk
// table camera-major (the device groups it into 8 point slices).
struct Runs {
  std::vector<int32_t> cam_off, cam_rng, wcam;
  std::vector<Chunk> chunks;
  int64_t npad = 0;
};
inline void camera_runs(int C, const int32_t* n_obs_of_cam, Runs* r) {
  r->cam_off.assign(size_t(C) + 1, 0);
  r->cam_rng.assign(2 * size_t(C), 0);
  int64_t npad = 0;
  for (int c = 0; c < C; ++c) {
    const int32_t n_c = n_obs_of_cam[c];
    r->cam_off[c + 1] = r->cam_off[c] + n_c;
    r->cam_rng[2 * c] = int32_t(npad);
    r->cam_rng[2 * c + 1] = int32_t(npad + n_c);
    npad += (n_c + 63) / 64 * 64;
  }
  r->npad = npad;
  r->wcam.assign(size_t(npad / 64) + 1, 0);
  for (int c = 0; c < C; ++c)
    for (int64_t w = r->cam_rng[2 * c] / 64;
         w < (int64_t(r->cam_rng[2 * c]) + r->cam_off[c + 1] - r->cam_off[c] + 63) / 64; ++w)
      r->wcam[size_t(w)] = c;
  r->chunks.clear();
  for (int c = 0; c < C; ++c) {
    const int32_t n_c = r->cam_off[c + 1] - r->cam_off[c];
    for (int32_t k = 0; 64 * k < n_c; ++k)
      r->chunks.push_back(Chunk{c, r->cam_rng[2 * c] + 64 * k, std::min<int32_t>(64, n_c - 64 * k),
                                r->cam_off[c] + 64 * k});
  }
}

// Small path: the chunk table's slice sizes from the host's per-camera slice
// counts (camera c's chunk k starts at its 64 k-th observation in point
// order, whose slice the counts' running sum gives) -> the largest slice.
inline int32_t small_slice_max(int C, const int32_t* n_obs_of_cam, const std::vector<int32_t>& cam_slice) {
  std::array<int32_t, 8> jcnt{};
  for (int c = 0; c < C; ++c) {
    const int32_t n_c = n_obs_of_cam[c];
    int32_t cum = 0;
    int sl = 0;
    for (int32_t k = 0; 64 * k < n_c; ++k) {
      while (sl < 7 && cum + cam_slice[8 * size_t(c) + sl] <= 64 * k) cum += cam_slice[8 * size_t(c) + sl++];
      ++jcnt[size_t(sl)];
    }
  }
  return *std::max_element(jcnt.begin(), jcnt.end());
}

}  // namespace hostlayout
}  // namespace sfm

#endif  // SFM_BA_HOST_LAYOUT_H_
