// CMap's observation store on the device: the map
// points, their (frame, keypoint) observations and their descriptor rows,
// resident in HBM, with the queries the live tracking path makes of CMap:
//
//   addNewPoints       CMap.cpp:36-78   points + one observation per frame,
//                                       emplaced point-major (i, then j)
//   addPointMatches    CMap.cpp:118-132 one observation per point
//   addDescriptors     CMap.cpp:308-315 one descriptor row per point
//   getPointsAtIdx     CMap.cpp:134-143 (and the BA write-back)
//   getPointsInFrames  CMap.cpp:277-295 sorted unique points seen in any of
//                                       the frames (CSfM.cpp:648)
//   getPointsInFrame   CMap.cpp:145-240 multimap equal_range order; for
//                                       every entry, EVERY 2D index the point
//                                       has in that frame (a point matched
//                                       twice in a frame yields 2 x 2)
//   getRepresentativeDescriptors  CMap.cpp:345-381 (CSfM.cpp:669)
//   updatePointViews / incrementMapAge   CMap.cpp:561-574
//   removePointsThreshold / removePoints CMap.cpp:384-474
//   removeFrame / arePointsSeenByAtLeast CMap.cpp:483-558
//   CSfM::cullKeyFrames                  CSfM.cpp:708-752 (one call)
//
// Layout: three row tables (RowTable, owner.h: observations, points,
// descriptor rows), each with one count and one capacity.  Observations are
// kept in global emplace order, which is taken as the multimap's order within
// one key (the reference's container is an unordered_multimap, CMap.h:96-97,
// whose equal_range order is implementation-defined; libc++, the reference's
// toolchain, keeps insertion order) and is the order of each point's
// _frameNo/_pts2DIdx lists.  Descriptor rows are kept in append order with
// their point.  The per-point CSRs (observations, descriptor rows) are
// rebuilt lazily by a stable radix sort after appends.  Queries are flag +
// stable compaction (hipcub DeviceSelect), so every result keeps the
// reference's order.  A call that changes the store reserves everything it
// can need first (Room, Removal), then enqueues, synchronises once and only
// then commits the counts and the live mirror and clears the CSR flags.
//
// Culling: every point carries _timeAlive / _kfAlive / _ptsViews (int32) and
// a live flag (membership of _pts3DIdx) beside X, every observation a flag
// for its _frameViewsPointIdx entry: removeFrame erases ALL of a frame's
// multimap entries but only the listed points' list entries, so the two can
// diverge, and the frame-keyed queries read the flag while the per-point
// lists (k_dup_count / k_dup_fill) do not.  Removals mark tombstones per
// observation and per descriptor row and end in one stable compaction of the
// arrays (hipcub scan + scatter), after which both CSRs are stale.  The cull
// rules and the keyframe loop's decisions are taken on the device; each call
// reads its results back with one host synchronisation.  A removed point
// keeps its slot and X (indices are never renumbered); the host mirror of
// the live flags lets the argument checks refuse it without a readback.
// With no culling call made every flag is 1 and every query is what it was.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "sfm_trace.h"
#include "map_internal.h"
#include "mappoint_internal.h"
#include "../../include/sfm_amd.h"
#include "dev_mem.h"

namespace sfm {
namespace {

int mapfail(int code, const std::string& m) { return fail(code, "sfm_map: " + m); }

__global__ void k_mark_frames(int64_t n, const int32_t* __restrict__ ob_pt, const int32_t* __restrict__ ob_frame,
                              const uint8_t* __restrict__ ob_mm, const int32_t* __restrict__ fset, int nf,
                              uint8_t* __restrict__ mark) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= n || !ob_mm[e]) return;  // (ob_mm: the observation still has its multimap entry)
  const int f = ob_frame[e];
  int lo = 0, hi = nf;  // fset ascending
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (fset[mid] < f) lo = mid + 1; else hi = mid;
  }
  if (lo < nf && fset[lo] == f) mark[ob_pt[e]] = 1;  // idempotent plain store
}

__global__ void k_flag_frame(int64_t n, const int32_t* __restrict__ ob_frame, const uint8_t* __restrict__ ob_mm, int f,
                             uint8_t* __restrict__ flag) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e < n) flag[e] = ob_frame[e] == f && ob_mm[e];
}

// rank of each observation's frame in the query list (fr sorted by frame,
// with the query position alongside), nf when the frame is not queried
__global__ void k_frame_rank(int64_t n, const int32_t* __restrict__ ob_frame, const uint8_t* __restrict__ ob_mm,
                             const int2* __restrict__ fr, int nf, uint32_t* __restrict__ key,
                             int32_t* __restrict__ iota) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int f = ob_frame[e];
  int lo = 0, hi = nf;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (fr[mid].x < f) lo = mid + 1; else hi = mid;
  }
  key[e] = uint32_t(lo < nf && fr[lo].x == f && ob_mm[e] ? fr[lo].y : nf);
  iota[e] = int32_t(e);
}

__global__ void k_count_keys(int64_t n, const int32_t* __restrict__ key, int32_t* __restrict__ cnt) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e < n) atomicAdd(cnt + key[e], 1);
}

__global__ void k_iota(int64_t n, int32_t* __restrict__ v) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e < n) v[e] = int32_t(e);
}

// entry e of the frame's equal range (observation sel[e] of point p): how
// many of p's observations are in frame f
__global__ void k_dup_count(int n_sel, const int32_t* __restrict__ sel, const int32_t* __restrict__ ob_pt,
                            const int32_t* __restrict__ ob_frame, const int32_t* __restrict__ orow,
                            const int32_t* __restrict__ ooff, int f, int32_t* __restrict__ cnt) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_sel) return;
  const int p = ob_pt[sel[e]];
  const int fe = f == INT32_MIN ? ob_frame[sel[e]] : f;  // INT32_MIN: the entry's own frame (multi-frame query)
  int c = 0;
  for (int q = ooff[p]; q < ooff[p + 1]; ++q) c += ob_frame[orow[q]] == fe;
  cnt[e] = c;
}

__global__ void k_dup_fill(int n_sel, const int32_t* __restrict__ sel, const int32_t* __restrict__ ob_pt,
                           const int32_t* __restrict__ ob_frame, const int32_t* __restrict__ ob_idx,
                           const int32_t* __restrict__ orow, const int32_t* __restrict__ ooff, int f,
                           const int32_t* __restrict__ off2, int32_t* __restrict__ out3, int32_t* __restrict__ out2) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_sel) return;
  const int p = ob_pt[sel[e]];
  const int fe = f == INT32_MIN ? ob_frame[sel[e]] : f;
  out3[e] = p;
  int w = off2[e];
  for (int q = ooff[p]; q < ooff[p + 1]; ++q) {
    const int o = orow[q];
    if (ob_frame[o] == fe) out2[w++] = ob_idx[o];
  }
}

// k_dup_count over the rank-sorted observations of a multi-frame query:
// entries of the queried frames (rank < nf) count their point's
// observations in their own frame, the rest 0
__global__ void k_dup_count_ranked(int64_t n, const int32_t* __restrict__ sel, const uint32_t* __restrict__ rank,
                                   int nf, const int32_t* __restrict__ ob_pt, const int32_t* __restrict__ ob_frame,
                                   const int32_t* __restrict__ orow, const int32_t* __restrict__ ooff,
                                   int32_t* __restrict__ cnt) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= n) return;
  int c = 0;
  if (int(rank[e]) < nf) {
    const int o = sel[e], p = ob_pt[o], f = ob_frame[o];
    for (int q = ooff[p]; q < ooff[p + 1]; ++q) c += ob_frame[orow[q]] == f;
  }
  cnt[e] = c;
}

// the frames' entry offsets (exclusive scan of the per-rank counts) and 2D
// offsets (the entry scan at each frame's first entry): offs[0..nf] and
// offs[nf+1 .. 2nf+1]
__global__ void k_frame_offsets(int nf, const int32_t* __restrict__ fcnt, int64_t n, const int32_t* __restrict__ cnt,
                                const int32_t* __restrict__ eoff, int32_t* __restrict__ offs) {
  const int32_t total2 = n ? eoff[n - 1] + cnt[n - 1] : 0;
  int32_t o = 0;
  for (int i = 0; i <= nf; ++i) {
    offs[i] = o;
    offs[nf + 1 + i] = o < n ? eoff[o] : total2;
    if (i < nf) o += fcnt[i];
  }
}

// one wave per queried point: the point's row (in append order) with the
// smallest sum of Hamming distances to its other rows, the first on ties
// (repr_row, mappoint_internal.h)
template <int W>
__global__ __launch_bounds__(64) void k_map_repr(const uint64_t* __restrict__ desc, const int32_t* __restrict__ drow,
                                                 const int32_t* __restrict__ doff, const int32_t* __restrict__ qpt,
                                                 int n, const int32_t* __restrict__ n_dev,
                                                 int32_t* __restrict__ best_local, uint64_t* __restrict__ out) {
  const int i = blockIdx.x, l = threadIdx.x;
  if (i >= (n_dev ? *n_dev : n)) return;  // (n_dev: the count on the device, n its bound)
  const int p = qpt[i];
  const int r0 = doff[p], k = doff[p + 1] - r0;
  if (k == 0) {  // no descriptor row (the callers check; reported as -1)
    if (l == 0) best_local[i] = -1;
    if (l < W) out[size_t(i) * W + l] = 0;
    return;
  }
  const int b = repr_row<W>(k, l, [=](int r) { return desc + size_t(drow[r0 + r]) * W; });
  if (l == 0) best_local[i] = b;
  if (l < W) out[size_t(i) * W + l] = desc[size_t(drow[r0 + b]) * W + l];
}

__global__ void k_scatter_points(int n, const int32_t* __restrict__ idx, const double* __restrict__ v,
                                 double* __restrict__ X) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t p = size_t(idx[i]) * 3;
  X[p] = v[3 * size_t(i)];
  X[p + 1] = v[3 * size_t(i) + 1];
  X[p + 2] = v[3 * size_t(i) + 2];
}

inline unsigned grid(int64_t n, int b = 256) { return unsigned((n + b - 1) / b); }

__global__ void k_gather_points(int n, const int32_t* __restrict__ idx, const double* __restrict__ X,
                                double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t p = size_t(idx[i]) * 3;
  out[3 * size_t(i)] = X[p];
  out[3 * size_t(i) + 1] = X[p + 1];
  out[3 * size_t(i) + 2] = X[p + 2];
}

__global__ void k_unmark(int n, const int32_t* __restrict__ pts, uint8_t* __restrict__ mark) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mark[pts[i]] = 0;
}

// ---- culling (CMap.cpp:384-574, CSfM.cpp:708-752)

__global__ void k_fill_i32(int n, int32_t* __restrict__ v, int32_t x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = x;
}

// _ptsViews[idx]++ per entry; repeats count (integer adds commute)
__global__ void k_add_views(int n, const int32_t* __restrict__ idx, int32_t* __restrict__ views) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(views + idx[i], 1);
}

__global__ void k_age(int P, const uint8_t* __restrict__ live, int32_t* __restrict__ time, int32_t* __restrict__ kf,
                      int t_inc, int kf_inc) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P || !live[p]) return;
  time[p] += t_inc;
  kf[p] += kf_inc;
}

__global__ void k_point_state(int n, const int32_t* __restrict__ idx, const int32_t* __restrict__ time,
                              const int32_t* __restrict__ kf, const int32_t* __restrict__ views,
                              const int32_t* __restrict__ ooff, const uint8_t* __restrict__ live,
                              int32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int p = idx[i];
  int32_t* o = out + 5 * size_t(i);
  o[0] = time[p];
  o[1] = kf[p];
  o[2] = views[p];
  o[3] = ooff[p + 1] - ooff[p];
  o[4] = live[p];
}

// CMap::removePointsThreshold's two rules (CMap.cpp:386-399); the score is
// the reference's float division, so timeAlive = 0 gives +inf (kept)
__global__ void k_cull_flag(int P, const uint8_t* __restrict__ live, const int32_t* __restrict__ time,
                            const int32_t* __restrict__ kf, const int32_t* __restrict__ views,
                            const int32_t* __restrict__ ooff, int kf_thr, float track_thr,
                            uint8_t* __restrict__ flag) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  bool cull = false;
  if (live[p]) {
    const int n_obs = ooff[p + 1] - ooff[p], k = kf[p];
    if (k >= 1 && k <= kf_thr) {
      const float score = float(views[p]) / float(time[p]);
      cull = n_obs < kf_thr || score < track_thr;
    }
    cull = cull || (n_obs < kf_thr && k > kf_thr);
  }
  flag[p] = cull;
}

__global__ void k_flag_list(int n, const int32_t* __restrict__ idx, uint8_t* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[idx[i]] = 1;
}

// CMap::removePoints (CMap.cpp:406-474) for the flagged points: out of
// _pts3DIdx, every observation and descriptor row of theirs a tombstone, the
// status -1.  Nothing happens when the count exceeds the caller's capacity
// (n_dev NULL: no bound).
__global__ void k_kill_points(int P, int64_t N, int64_t rows, const uint8_t* __restrict__ flag,
                              const int32_t* __restrict__ n_dev, int capacity, const int32_t* __restrict__ ob_pt,
                              const int32_t* __restrict__ desc_pt, uint8_t* __restrict__ live,
                              uint8_t* __restrict__ odead, uint8_t* __restrict__ ddead, int32_t* __restrict__ status) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool apply = !n_dev || *n_dev <= capacity;
  if (e < P) {
    const bool c = flag[e] && apply;
    if (c) live[e] = 0;
    status[e] = c ? -1 : 0;
  }
  if (!apply) return;
  if (e < N && flag[ob_pt[e]]) odead[e] = 1;
  if (e < rows && flag[desc_pt[e]]) ddead[e] = 1;
}

__global__ void k_keep(int64_t n, const uint8_t* __restrict__ dead, int32_t* __restrict__ keep) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e < n) keep[e] = dead[e] == 0;
}

__global__ void k_compact_obs(int64_t n, const uint8_t* __restrict__ dead, const int32_t* __restrict__ pos,
                              const int32_t* __restrict__ pt, const int32_t* __restrict__ fr,
                              const int32_t* __restrict__ ix, const uint8_t* __restrict__ mm, int32_t* __restrict__ pt2,
                              int32_t* __restrict__ fr2, int32_t* __restrict__ ix2, uint8_t* __restrict__ mm2) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= n || dead[e]) return;
  const int q = pos[e];
  pt2[q] = pt[e];
  fr2[q] = fr[e];
  ix2[q] = ix[e];
  mm2[q] = mm[e];
}

__global__ void k_compact_desc(int64_t rows, int W, const uint8_t* __restrict__ dead, const int32_t* __restrict__ pos,
                               const uint64_t* __restrict__ desc, const int32_t* __restrict__ dpt,
                               uint64_t* __restrict__ desc2, int32_t* __restrict__ dpt2) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t r = t / W;
  const int w = int(t % W);
  if (r >= rows || dead[r]) return;
  const int q = pos[r];
  desc2[size_t(q) * W + w] = desc[size_t(r) * W + w];
  if (w == 0) dpt2[q] = dpt[r];
}

// tot = (observations kept, descriptor rows kept)
__global__ void k_totals(int64_t N, int64_t rows, const int32_t* __restrict__ okeep, const int32_t* __restrict__ opos,
                         const int32_t* __restrict__ dkeep, const int32_t* __restrict__ dpos,
                         int32_t* __restrict__ tot) {
  tot[0] = N ? opos[N - 1] + okeep[N - 1] : 0;
  tot[1] = rows ? dpos[rows - 1] + dkeep[rows - 1] : 0;
}

__global__ void k_nobs(int P, const int32_t* __restrict__ ooff, int32_t* __restrict__ nobs) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < P) nobs[p] = ooff[p + 1] - ooff[p];
}

// entry j (0-based) of a point's list = the j-th row of its CSR range that is
// not a tombstone; -1 past the end
__device__ inline int nth_live(const int32_t* row, const uint8_t* dead, int b, int e, int j) {
  for (int q = b; q < e; ++q) {
    const int o = row[q];
    if (dead[o]) continue;
    if (j-- == 0) return o;
  }
  return -1;
}

struct KfWalk {
  int n_walk, mode;  // mode 0: CSfM::cullKeyFrames; 1: removeFrame (no decision); 2: the decision alone
  int n_frames;      // arePointsSeenByAtLeast's nFramesThreshold
  const int32_t *frame_no, *off, *pts, *thr;  // per keyframe: its number, its list pts[off[k] .. off[k+1]), ceil(ratio n)
  const int32_t *ob_frame, *orow, *ooff, *drow, *doff;
  uint8_t *odead, *ddead, *own;
  int32_t *nobs, *views, *cnt, *culled, *err;  // err: (set, keyframe, point, frame)
};

// The greedy loop of CSfM::cullKeyFrames (CSfM.cpp:708-752) in one workgroup,
// keyframe after keyframe with no host round trip: the decision of
// CMap::arePointsSeenByAtLeast (CMap.cpp:544-558) reads only the points' list
// lengths (nobs, kept current here), and CMap::removeFrame's per-point part
// (CMap.cpp:486-522) touches only the listed points' own rows.  A point
// listed k times is handled by ONE lane (the entry whose atomic count came
// back 0) doing k removals in sequence, each with std::lower_bound's
// bisection on the point's list as it then stands.  Removals are first
// marked pending (2): when any entry fails the reference's unchecked
// assumptions the keyframe's marks are withdrawn, the error is recorded and
// the walk ends; otherwise they become tombstones (1) and the counters move.
// The multimap erase of the culled frames and the compaction follow on a
// full grid (k_clear_mm, compact).
__global__ __launch_bounds__(1024) void k_walk_keyframes(KfWalk a) {
  __shared__ int s_cnt, s_fail;
  const int tid = threadIdx.x, T = blockDim.x;
  for (int k = 0; k < a.n_walk; ++k) {
    const int b = a.off[k], e = a.off[k + 1], f = a.frame_no[k];
    if (tid == 0) { s_cnt = 0; s_fail = INT_MAX; }
    __syncthreads();
    bool cull = a.mode == 1;
    if (!cull) {
      int c = 0;
      for (int i = b + tid; i < e; i += T) c += a.nobs[a.pts[i]] > a.n_frames;
      for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
      if ((tid & 63) == 0 && c) atomicAdd(&s_cnt, c);
      __syncthreads();
      cull = s_cnt > a.thr[k];
    }
    if (a.mode == 2 || !cull) {
      if (tid == 0) a.culled[k] = cull;
      __syncthreads();  // (s_cnt is read above, reset below)
      continue;
    }
    // one owner per distinct point
    for (int i = b + tid; i < e; i += T) a.own[i] = atomicAdd(a.cnt + a.pts[i], 1) == 0;
    __syncthreads();
    for (int i = b + tid; i < e; i += T) {
      if (!a.own[i]) continue;
      const int p = a.pts[i], m = atomicAdd(a.cnt + p, 0);  // (read where the adds above were made)
      const int ob = a.ooff[p], oe = a.ooff[p + 1], db = a.doff[p], de = a.doff[p + 1];
      int len = 0, dlen = 0;
      for (int q = ob; q < oe; ++q) len += a.odead[a.orow[q]] == 0;
      for (int q = db; q < de; ++q) dlen += a.ddead[a.drow[q]] == 0;
      for (int r = 0; r < m; ++r) {
        int first = 0, count = len;  // std::lower_bound(_frameNo[p].begin(), .end(), frameNo)
        while (count > 0) {
          const int step = count >> 1;
          if (a.ob_frame[nth_live(a.orow, a.odead, ob, oe, first + step)] < f) {
            first += step + 1;
            count -= step + 1;
          } else {
            count = step;
          }
        }
        const int o = first < len ? nth_live(a.orow, a.odead, ob, oe, first) : -1;
        if (o < 0 || a.ob_frame[o] != f || dlen <= first) {
          atomicMin(&s_fail, i);
          break;
        }
        a.odead[o] = 2;
        a.ddead[nth_live(a.drow, a.ddead, db, de, first)] = 2;
        --len;
        --dlen;
      }
    }
    __syncthreads();
    const int fail = s_fail;
    for (int i = b + tid; i < e; i += T) {
      if (!a.own[i]) continue;
      const int p = a.pts[i];
      int gone = 0;
      for (int q = a.ooff[p]; q < a.ooff[p + 1]; ++q) {
        const int o = a.orow[q];
        if (a.odead[o] == 2) { a.odead[o] = fail == INT_MAX; ++gone; }
      }
      for (int q = a.doff[p]; q < a.doff[p + 1]; ++q) {
        const int d = a.drow[q];
        if (a.ddead[d] == 2) a.ddead[d] = fail == INT_MAX;
      }
      if (fail == INT_MAX) {  // _frameNo[p] shrinks, _ptsViews[p]-- per removal
        a.nobs[p] -= gone;
        a.views[p] -= gone;
      }
    }
    __syncthreads();  // (every lane has read its own[i] and cnt)
    for (int i = b + tid; i < e; i += T) a.cnt[a.pts[i]] = 0;
    if (tid == 0) {
      a.culled[k] = fail == INT_MAX;
      if (fail != INT_MAX) { a.err[0] = 1; a.err[1] = k; a.err[2] = a.pts[fail]; a.err[3] = f; }
    }
    __syncthreads();
    if (fail != INT_MAX) break;
  }
}

// _frameViewsPointIdx.erase(frameNo) for the culled keyframes (CMap.cpp:525):
// every surviving observation of such a frame loses its multimap entry, the
// unlisted points' included
__global__ void k_clear_mm(int64_t N, const int32_t* __restrict__ ob_frame, const uint8_t* __restrict__ odead, int n_kf,
                           const int32_t* __restrict__ frame_no, const int32_t* __restrict__ culled,
                           uint8_t* __restrict__ mm) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= N || odead[e]) return;
  const int f = ob_frame[e];
  for (int k = 0; k < n_kf; ++k)
    if (culled[k] && frame_no[k] == f) { mm[e] = 0; return; }
}

// The queried points projected with the frame's pose (CSfM.cpp:664-668, the
// reference's GeometryUtils::projectPoints with zero distortion, as
// sfm_amd/live.py's _project): uv = (x / z) f + c.
__global__ void k_project(int n, const int32_t* __restrict__ n_dev, const int32_t* __restrict__ qpt,
                          const double* __restrict__ X, double r0, double r1,
                          double r2, double r3, double r4, double r5, double r6, double r7, double r8, double t0,
                          double t1, double t2, double fx, double fy, double cx, double cy, double* __restrict__ uv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (n_dev ? *n_dev : n)) return;
  const double* x = X + 3 * size_t(qpt[i]);
  const double x0 = x[0], x1 = x[1], x2 = x[2];
  const double c0 = r0 * x0 + r1 * x1 + r2 * x2 + t0;
  const double c1 = r3 * x0 + r4 * x1 + r5 * x2 + t1;
  const double c2 = r6 * x0 + r7 * x1 + r8 * x2 + t2;
  uv[2 * size_t(i)] = c0 / c2 * fx + cx;
  uv[2 * size_t(i) + 1] = c1 / c2 * fy + cy;
}

}  // namespace
// match_kernels.hip
int matcher_match_current_dev(sfm_matcher* h, hipEvent_t after, const uint64_t* q, const double* p0, int n0,
                              const int32_t* d_n0, const int32_t* d_train_idx, int n1, double ratio, double mn,
                              double mx, int** res);
int matcher_current_n(const sfm_matcher* h);
int matcher_words(const sfm_matcher* h);
int matcher_device(const sfm_matcher* h);
int matcher_keyframe_rows(sfm_matcher* h, int32_t slot, const uint64_t** desc, int* n, hipEvent_t* ready);
}  // namespace sfm

using namespace sfm;

// The stream first: members are destroyed in reverse order, so it goes last.
struct sfm_map {
  explicit sfm_map(int words) : W(words), rows({sizeof(uint64_t) * size_t(words), sizeof(int32_t)}) {}
  Stream s;
  int device = 0, W;
  RowTable<DeviceMem, 4> obs{{4, 4, 4, 1}};      // observations, emplace order
  RowTable<DeviceMem, 5> pts{{24, 4, 4, 4, 1}};  // point slots; n() is the number of points ever added
  RowTable<DeviceMem, 2> rows;                    // descriptor rows, append order
  std::vector<uint8_t> live_h;                    // pt_live's host mirror (argument checks make no readback)
  int32_t n_live = 0;
  bool ocsr = false, dcsr = false;                // per-point CSRs current?
  int32_t *orow = nullptr, *ooff = nullptr, *drow = nullptr, *doff = nullptr;  // (views into scratch: build_csr)
  std::map<std::string, DevBuf> scratch;
  Event ev;                                       // sfm_map_match_frame: its queries are ready
  PinArr<int32_t> pin;                            // the handle's pinned block (pin_reserve)

  int32_t n_pts() const { return int32_t(pts.n()); }
  int32_t* ob_pt() const { return obs.col<int32_t>(0); }
  int32_t* ob_frame() const { return obs.col<int32_t>(1); }
  int32_t* ob_idx() const { return obs.col<int32_t>(2); }
  uint8_t* ob_mm() const { return obs.col<uint8_t>(3); }  // 1: the observation's _frameViewsPointIdx entry exists
  double* X() const { return pts.col<double>(0); }        // [n_pts][3]
  int32_t* pt_time() const { return pts.col<int32_t>(1); }   // _timeAlive
  int32_t* pt_kf() const { return pts.col<int32_t>(2); }     // _kfAlive
  int32_t* pt_views() const { return pts.col<int32_t>(3); }  // _ptsViews
  uint8_t* pt_live() const { return pts.col<uint8_t>(4); }   // 1: the point is in _pts3DIdx
  uint64_t* desc() const { return rows.col<uint64_t>(0); }   // [rows][W]
  int32_t* desc_pt() const { return rows.col<int32_t>(1); }  // point of each row
};

namespace {

// the scratch buffer `name`, at least count T (contents dropped when it grows)
template <class T = uint8_t>
T* scratch(sfm_map* h, const char* name, size_t count, int* rc) {
  DevBuf& b = h->scratch[name];
  // grow by half again at least: the map grows every keyframe, and a
  // reallocation costs a stream synchronisation plus hipFree / hipMalloc
  const size_t bytes = sizeof(T) * count, want = std::max<size_t>({bytes, b.bytes() + b.bytes() / 2, 256});
  if (b.reserve(std::max<size_t>(bytes, 1), want, h->s))
    *rc = mapfail(SFM_ENOMEM, std::string("hipMalloc failed (") + name + ")");
  return b.as<T>();
}

// The handle's pinned block, at least n ints (grown while the stream is idle).
int32_t* pin_reserve(sfm_map* h, size_t n, int* rc) {
  if (h->pin.reserve(sizeof(int32_t) * n, sizeof(int32_t) * (std::max<size_t>(n, 8192) * 3 / 2), h->s))
    *rc = mapfail(SFM_ENOMEM, "hipHostMalloc failed");
  return h->pin;
}
int sync(sfm_map* h) {
  return hipStreamSynchronize(h->s) == hipSuccess ? 0 : mapfail(SFM_EIO, "kernel or copy failed");
}

// ---- the device primitives.  f(temporary, bytes) is a hipcub call: the size
// query (host only, no data pointer read), the temporary from scratch `tag`,
// the call.  run = false reserves: the later run with that tag and n allocates nothing.
template <class F>
int cub(sfm_map* h, const char* tag, bool run, const char* what, F f) {
  int rc = 0;
  size_t bytes = 0;
  (void)f(nullptr, bytes);
  void* tmp = scratch(h, tag, bytes, &rc);
  if (rc || !run) return rc;
  return f(tmp, bytes) == hipSuccess ? 0 : mapfail(SFM_EIO, what);
}
int exclusive_sum(sfm_map* h, const char* tag, const int32_t* in, int32_t* out, int n, bool run = true) {
  return cub(h, tag, run, "scan failed",
             [=](void* p, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(p, b, in, out, n, h->s); });
}
// out[0 .. *n_out) = the indices i < n with flag[i] set, ascending (n_out on the device)
int select_flagged(sfm_map* h, const char* tag, const uint8_t* flag, int32_t* out, int32_t* n_out, int n,
                   bool run = true) {
  const hipcub::CountingInputIterator<int32_t> iota(0);
  return cub(h, tag, run, "select failed",
             [=](void* p, size_t& b) { return hipcub::DeviceSelect::Flagged(p, b, iota, flag, out, n_out, n, h->s); });
}
// stable: (key, val) sorted by the keys' low `bits` bits into (key2, val2)
int sort_pairs(sfm_map* h, const char* tag, const uint32_t* key, uint32_t* key2, const int32_t* val, int32_t* val2,
               int n, int bits, const char* what) {
  return cub(h, tag, true, what, [=](void* p, size_t& b) {
    return hipcub::DeviceRadixSort::SortPairs(p, b, key, key2, val, val2, n, 0, bits, h->s);
  });
}

// CSR by point of `key` (n entries, keys < P): rows (entry ids grouped by
// key, ascending within a key = append order) and offsets [P+1].  *current is
// set once the rebuild is enqueued (scratch, an in-order stream), cleared by
// the commit that stales it.
int build_csr(sfm_map* h, bool* current, const char* tag, const int32_t* key, int64_t n, int32_t** rows_out,
              int32_t** off_out) {
  if (*current) return 0;
  int rc = 0;
  const int P = h->n_pts();
  const std::string t(tag);
  const size_t n1 = size_t(std::max<int64_t>(n, 1));
  auto* kk = scratch<uint32_t>(h, (t + "k").c_str(), n1, &rc);
  auto* iv = scratch<int32_t>(h, (t + "i").c_str(), n1, &rc);
  auto* rows = scratch<int32_t>(h, (t + "r").c_str(), n1, &rc);
  auto* cnt = scratch<int32_t>(h, (t + "c").c_str(), size_t(P) + 1, &rc);
  auto* off = scratch<int32_t>(h, (t + "o").c_str(), size_t(P) + 1, &rc);
  if (rc) return rc;
  (void)hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t(P) + 1), h->s);
  if (n) {
    k_count_keys<<<grid(n), 256, 0, h->s>>>(n, key, cnt);
    k_iota<<<grid(n), 256, 0, h->s>>>(n, iv);
    int bits = 1;
    while (bits < 32 && (1ll << bits) < P) ++bits;
    if (int r = sort_pairs(h, (t + "t").c_str(), reinterpret_cast<const uint32_t*>(key), kk, iv, rows, int(n), bits,
                           "radix sort failed"))
      return r;
  }
  if (int r = exclusive_sum(h, (t + "s").c_str(), cnt, off, P + 1)) return r;
  *rows_out = rows;
  *off_out = off;
  *current = true;
  return 0;
}
int ensure_ocsr(sfm_map* h) { return build_csr(h, &h->ocsr, "ob", h->ob_pt(), h->obs.n(), &h->orow, &h->ooff); }
int ensure_dcsr(sfm_map* h) { return build_csr(h, &h->dcsr, "de", h->desc_pt(), h->rows.n(), &h->drow, &h->doff); }
int ensure_csrs(sfm_map* h) {
  const int rc = ensure_ocsr(h);
  return rc ? rc : ensure_dcsr(h);
}

// in range and still in the map (a removed point keeps its slot and its X,
// and is refused everywhere but sfm_map_get_points / sfm_map_set_points)
int check_pts(const sfm_map* h, int32_t n, const int32_t* idx, bool live = false) {
  for (int32_t i = 0; i < n; ++i) {
    if (idx[i] < 0 || idx[i] >= h->n_pts())
      return mapfail(SFM_EINVAL, "point index " + std::to_string(idx[i]) + " out of range at " + std::to_string(i));
    if (live && !h->live_h[size_t(idx[i])])
      return mapfail(SFM_EINVAL, "point " + std::to_string(idx[i]) + " (at " + std::to_string(i) + ") was removed");
  }
  return 0;
}

// The opening of a call over a point list (args: its arrays are there): (rc, go).  go: the device is set;
// else the call ends with rc (0 when n = 0).
std::pair<int, bool> open_list(sfm_map* h, int32_t n, const int32_t* idx, bool args, bool live) {
  if (!h) return {mapfail(SFM_EINVAL, "NULL handle"), false};
  if (n <= 0) return {n < 0 ? mapfail(SFM_EINVAL, "negative size") : 0, false};
  if (!args) return {mapfail(SFM_EINVAL, "NULL argument"), false};
  if (int rc = check_pts(h, n, idx, live)) return {rc, false};
  if (hipSetDevice(h->device) != hipSuccess) return {mapfail(SFM_ENODEV, "hipSetDevice failed"), false};
  return {0, true};
}

// Appends.  A Room exists only by growing all three tables for what a call
// appends; a failed growth leaves every table as it was.  put / fill write
// the rows past the counts; rc keeps the first failure and stops the rest.
struct Room {
  sfm_map* h;
  int rc = 0;
  Room(sfm_map* h, int64_t n_obs, int64_t n_pts, int64_t n_rows) : h(h) {
    if (h->obs.reserve(h->obs.n() + n_obs, h->s) || h->pts.reserve(h->pts.n() + n_pts, h->s) ||
        h->rows.reserve(h->rows.n() + n_rows, h->s))
      rc = mapfail(SFM_ENOMEM, "hipMalloc failed (growth)");
  }
  template <class T>
  void put(T* dst, const T* src, int64_t n) {
    if (!rc && n && hipMemcpyAsync(dst, src, size_t(n) * sizeof(T), hipMemcpyHostToDevice, h->s) != hipSuccess)
      rc = mapfail(SFM_EIO, "upload failed");
  }
  template <class T>  // n entries of `value` (a byte pattern: 0, or 1 for the byte arrays)
  void fill(T* dst, int value, int64_t n) {
    if (!rc && n && hipMemsetAsync(dst, value, size_t(n) * sizeof(T), h->s) != hipSuccess)
      rc = mapfail(SFM_EIO, "memset failed");
  }
};

// Removals.  Everything one can need, taken before its first write to the
// store: the tombstones (per observation and descriptor row: 0 kept, 1
// removed, 2 pending inside k_walk_keyframes), the pinned block of n_pin ints
// and, with `compacting`, compact's ten arrays and its two scans' temporaries.
struct Removal {
  int rc = 0;
  int64_t N, rows;
  uint8_t *odead, *ddead, *mm2;
  int32_t *okeep, *opos, *dkeep, *dpos, *pt2, *fr2, *ix2, *dpt2, *pin;
  uint64_t* desc2;
  Removal(sfm_map* h, size_t n_pin, bool compacting = true) : N(h->obs.n()), rows(h->rows.n()) {
    const size_t n1 = size_t(std::max<int64_t>(N, 1)), r1 = size_t(std::max<int64_t>(rows, 1));
    odead = scratch<uint8_t>(h, "odead", n1, &rc);
    ddead = scratch<uint8_t>(h, "ddead", r1, &rc);
    pin = pin_reserve(h, n_pin, &rc);
    if (!compacting) return;
    okeep = scratch<int32_t>(h, "cok", n1, &rc);
    opos = scratch<int32_t>(h, "cop", n1, &rc);
    dkeep = scratch<int32_t>(h, "cdk", r1, &rc);
    dpos = scratch<int32_t>(h, "cdp", r1, &rc);
    pt2 = scratch<int32_t>(h, "cpt", n1, &rc);
    fr2 = scratch<int32_t>(h, "cfr", n1, &rc);
    ix2 = scratch<int32_t>(h, "cix", n1, &rc);
    mm2 = scratch<uint8_t>(h, "cmm", n1, &rc);
    desc2 = scratch<uint64_t>(h, "cde", r1 * h->W, &rc);
    dpt2 = scratch<int32_t>(h, "cdq", r1, &rc);
    if (int r = N ? exclusive_sum(h, "cos", okeep, opos, int(N), false) : 0) rc = r;
    if (int r = rows ? exclusive_sum(h, "cds", dkeep, dpos, int(rows), false) : 0) rc = r;
  }
};

void tomb_clear(sfm_map* h, const Removal& m) {
  (void)hipMemsetAsync(m.odead, 0, size_t(std::max<int64_t>(m.N, 1)), h->s);
  (void)hipMemsetAsync(m.ddead, 0, size_t(std::max<int64_t>(m.rows, 1)), h->s);
}

// One stable compaction of the observation table and of the descriptor rows
// past the call's tombstones, enqueued on the stream: keep flags, their
// exclusive scan (hipcub), a scatter into scratch copies, and the copies back.
// tot (device, 2 ints) receives the new sizes; the caller reads them with its
// one readback and passes them to compact_done.
int compact(sfm_map* h, const Removal& m, int32_t* tot) {
  const int64_t N = m.N, rows = m.rows;
  if (N) {
    k_keep<<<grid(N), 256, 0, h->s>>>(N, m.odead, m.okeep);
    if (int r = exclusive_sum(h, "cos", m.okeep, m.opos, int(N))) return r;
    k_compact_obs<<<grid(N), 256, 0, h->s>>>(N, m.odead, m.opos, h->ob_pt(), h->ob_frame(), h->ob_idx(), h->ob_mm(),
                                             m.pt2, m.fr2, m.ix2, m.mm2);
    (void)hipMemcpyAsync(h->ob_pt(), m.pt2, sizeof(int32_t) * size_t(N), hipMemcpyDeviceToDevice, h->s);
    (void)hipMemcpyAsync(h->ob_frame(), m.fr2, sizeof(int32_t) * size_t(N), hipMemcpyDeviceToDevice, h->s);
    (void)hipMemcpyAsync(h->ob_idx(), m.ix2, sizeof(int32_t) * size_t(N), hipMemcpyDeviceToDevice, h->s);
    (void)hipMemcpyAsync(h->ob_mm(), m.mm2, size_t(N), hipMemcpyDeviceToDevice, h->s);
  }
  if (rows) {
    k_keep<<<grid(rows), 256, 0, h->s>>>(rows, m.ddead, m.dkeep);
    if (int r = exclusive_sum(h, "cds", m.dkeep, m.dpos, int(rows))) return r;
    k_compact_desc<<<grid(rows * h->W), 256, 0, h->s>>>(rows, h->W, m.ddead, m.dpos, h->desc(), h->desc_pt(), m.desc2,
                                                        m.dpt2);
    (void)hipMemcpyAsync(h->desc(), m.desc2, sizeof(uint64_t) * size_t(rows) * h->W, hipMemcpyDeviceToDevice, h->s);
    (void)hipMemcpyAsync(h->desc_pt(), m.dpt2, sizeof(int32_t) * size_t(rows), hipMemcpyDeviceToDevice, h->s);
  }
  k_totals<<<1, 1, 0, h->s>>>(N, rows, m.okeep, m.opos, m.dkeep, m.dpos, tot);
  return 0;
}

void compact_done(sfm_map* h, const int32_t* tot) {
  if (tot[0] == h->obs.n() && tot[1] == h->rows.n()) return;  // nothing left: the CSRs stand
  h->obs.truncate(tot[0]);
  h->rows.truncate(tot[1]);
  h->ocsr = h->dcsr = false;
}

// The flagged points' removal and the compaction, enqueued (res: count,
// tot[2], list [P], status [P] on the device)
int kill_and_compact(sfm_map* h, const Removal& m, const uint8_t* flag, const int32_t* n_dev, int capacity,
                     int32_t* res) {
  const int P = h->n_pts();
  tomb_clear(h, m);
  k_kill_points<<<grid(std::max<int64_t>({P, m.N, m.rows})), 256, 0, h->s>>>(
      P, m.N, m.rows, flag, n_dev, capacity, h->ob_pt(), h->desc_pt(), h->pt_live(), m.odead, m.ddead, res + 3 + P);
  return compact(h, m, res + 1);
}

// CSfM::cullKeyFrames (mode 0), CMap::removeFrame (1) and
// CMap::arePointsSeenByAtLeast (2) over the keyframes' lists: one host
// synchronisation, the decisions and the removals on the device
int walk_keyframes(sfm_map* h, int mode, int32_t n_kf, const int32_t* frame_no, const int32_t* off, const int32_t* pts,
                   int32_t n_frames, double ratio, int32_t* culled) {
  if (!h) return mapfail(SFM_EINVAL, "NULL handle");
  if (n_kf < 0) return mapfail(SFM_EINVAL, "negative size");
  if (n_kf == 0) return 0;
  if (!frame_no || !off || !culled) return mapfail(SFM_EINVAL, "NULL argument");
  if (off[0] != 0) return mapfail(SFM_EINVAL, "off[0] must be 0");
  for (int k = 0; k < n_kf; ++k)
    if (off[k + 1] < off[k]) return mapfail(SFM_EINVAL, "off must not decrease");
  const int32_t total = off[n_kf];
  if (total && !pts) return mapfail(SFM_EINVAL, "NULL point list");
  if (int rc = check_pts(h, total, pts, true)) return rc;
  if (mode != 1 && !(ratio == ratio)) return mapfail(SFM_EINVAL, "ratio is NaN");
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  if (int rc = ensure_csrs(h)) return rc;
  int rc = 0;
  const int P = h->n_pts();
  const int64_t N = h->obs.n();
  // one upload: frame numbers, offsets, thresholds, lists
  std::vector<int32_t> in(frame_no, frame_no + n_kf);
  in.insert(in.end(), off, off + n_kf + 1);
  for (int k = 0; k < n_kf; ++k) {
    // int ptsThreshold = ceil(ratioPtsThreshold * pts3DIdx.size()), the product in double (CMap.cpp:546)
    const double v = mode == 1 ? 0.0 : std::ceil(ratio * double(off[k + 1] - off[k]));
    in.push_back(v >= double(INT_MAX) ? INT_MAX : v <= double(INT_MIN) ? INT_MIN : int32_t(v));
  }
  if (total) in.insert(in.end(), pts, pts + total);
  const size_t nres = size_t(n_kf) + 6;  // culled [n_kf], err [4], the sizes after [2]
  auto* din = scratch<int32_t>(h, "kin", in.size(), &rc);
  auto* res = scratch<int32_t>(h, "kres", nres, &rc);
  auto* nobs = scratch<int32_t>(h, "knobs", size_t(std::max(P, 1)), &rc);
  auto* cnt = scratch<int32_t>(h, "kcnt", size_t(std::max(P, 1)), &rc);
  auto* own = scratch<uint8_t>(h, "kown", size_t(std::max(total, 1)), &rc);
  if (rc) return rc;
  const Removal m(h, nres, mode != 2);
  if (m.rc) return m.rc;
  if (hipMemcpyAsync(din, in.data(), sizeof(int32_t) * in.size(), hipMemcpyHostToDevice, h->s) != hipSuccess)
    return mapfail(SFM_EIO, "upload failed");
  tomb_clear(h, m);
  (void)hipMemsetAsync(res, 0, sizeof(int32_t) * nres, h->s);
  (void)hipMemsetAsync(cnt, 0, sizeof(int32_t) * size_t(std::max(P, 1)), h->s);
  if (P) k_nobs<<<grid(P), 256, 0, h->s>>>(P, h->ooff, nobs);
  KfWalk a;
  a.n_walk = mode == 0 ? n_kf - 1 : n_kf;  // (the newest keyframe is never tried, CSfM.cpp:716)
  a.mode = mode;
  a.n_frames = n_frames;
  a.frame_no = din;
  a.off = din + n_kf;
  a.thr = din + 2 * size_t(n_kf) + 1;
  a.pts = din + 3 * size_t(n_kf) + 1;
  a.ob_frame = h->ob_frame();
  a.orow = h->orow;
  a.ooff = h->ooff;
  a.drow = h->drow;
  a.doff = h->doff;
  a.odead = m.odead;
  a.ddead = m.ddead;
  a.own = own;
  a.nobs = nobs;
  a.views = h->pt_views();
  a.cnt = cnt;
  a.culled = res;
  a.err = res + n_kf;
  if (a.n_walk > 0) k_walk_keyframes<<<1, 1024, 0, h->s>>>(a);
  if (mode != 2) {
    if (N) k_clear_mm<<<grid(N), 256, 0, h->s>>>(N, h->ob_frame(), m.odead, n_kf, a.frame_no, res, h->ob_mm());
    if (int r = compact(h, m, res + n_kf + 4)) return r;
  }
  const int32_t* ph = m.pin;
  (void)hipMemcpyAsync(m.pin, res, sizeof(int32_t) * nres, hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  if (mode != 2) compact_done(h, ph + n_kf + 4);
  std::memcpy(culled, ph, sizeof(int32_t) * size_t(n_kf));
  const int32_t* err = ph + n_kf;
  if (err[0])
    return mapfail(SFM_EINVAL, "removeFrame(" + std::to_string(err[3]) + "): point " + std::to_string(err[2]) +
                                   " of keyframe " + std::to_string(err[1]) +
                                   " does not hold the frame (with a descriptor row) where the bisection of its "
                                   "frame list ends; this keyframe was left as it was");
  return 0;
}

// getPointsInFrames, enqueued, all on the device: the points with an observation (its multimap entry
// standing) in any of the frames fset[0 .. nf) (ascending), minus the points minus[0 .. n_minus),
// ascending in out[0 .. *dn) (out holds n_pts ints).
int select_points_in_frames(sfm_map* h, const int32_t* fset, int nf, const int32_t* minus, int n_minus, int32_t* out,
                            int32_t* dn) {
  int rc = 0;
  const int P = h->n_pts();
  auto* mark = scratch<uint8_t>(h, "mark", size_t(P), &rc);
  if (rc) return rc;
  (void)hipMemsetAsync(mark, 0, size_t(P), h->s);
  k_mark_frames<<<grid(h->obs.n()), 256, 0, h->s>>>(h->obs.n(), h->ob_pt(), h->ob_frame(), h->ob_mm(), fset, nf, mark);
  if (n_minus) k_unmark<<<grid(n_minus), 256, 0, h->s>>>(n_minus, minus, mark);
  return select_flagged(h, "psel", mark, out, dn, P);
}

// k_map_repr for the handle's descriptor width
int launch_map_repr(sfm_map* h, int n, const int32_t* qpt, const int32_t* n_dev, int32_t* best, uint64_t* out) {
  switch (h->W) {
#define CASE(w) case w: k_map_repr<w><<<n, 64, 0, h->s>>>(h->desc(), h->drow, h->doff, qpt, n, n_dev, best, out); break;
    CASE(1) CASE(2) CASE(4) CASE(8) CASE(16) CASE(32) CASE(64)
#undef CASE
    default: return mapfail(SFM_EINVAL, "descriptor width");  // excluded by sfm_map_create
  }
  return 0;
}

}  // namespace

extern "C" {

int sfm_map_create(int32_t device, int32_t desc_bytes, sfm_map** out) {
  if (!out) return mapfail(SFM_EINVAL, "out is NULL");
  *out = nullptr;
  if (desc_bytes <= 0 || desc_bytes > 512 || desc_bytes % 8 || ((desc_bytes / 8) & (desc_bytes / 8 - 1)))
    return mapfail(SFM_EINVAL, "desc_bytes must be 8 x a power of two, <= 512 (BRISK: 64, ORB: 32)");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return mapfail(SFM_ENODEV, "no such device");
  if (hipSetDevice(device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  auto* h = new sfm_map(desc_bytes / 8);
  h->device = device;
  if (h->s.create(hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return mapfail(SFM_EIO, "hipStreamCreate failed");
  }
  *out = h;
  return 0;
}

int sfm_map_destroy(sfm_map* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->s);
  delete h;
  return 0;
}

int sfm_map_size(sfm_map* h, int32_t* n_pts, int64_t* n_obs, int64_t* n_desc_rows) {
  if (!h) return mapfail(SFM_EINVAL, "NULL handle");
  if (n_pts) *n_pts = h->n_pts();
  if (n_obs) *n_obs = h->obs.n();
  if (n_desc_rows) *n_desc_rows = h->rows.n();
  return 0;
}

int sfm_map_add_new_points(sfm_map* h, int32_t n_pts, const double* pts3d, int32_t n_frames, const int32_t* frame_no,
                           const int32_t* pts2d_idx, int32_t* pts3d_idx) {
  SFM_TRACE("sfm_map_add_new_points");
  if (!h) return mapfail(SFM_EINVAL, "NULL handle");
  if (n_pts < 0 || n_frames < 0) return mapfail(SFM_EINVAL, "negative size");
  if (n_pts == 0) return 0;
  if (!pts3d || (n_frames && (!frame_no || !pts2d_idx))) return mapfail(SFM_EINVAL, "NULL argument");
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  // emplace order of CMap.cpp:50-68: point i, then its frames j
  const int64_t m = int64_t(n_pts) * n_frames, N = h->obs.n();
  const int32_t P = h->n_pts();
  std::vector<int32_t> pt(m), fr(m), ix(m);
  for (int32_t i = 0; i < n_pts; ++i)
    for (int32_t j = 0; j < n_frames; ++j) {
      const int64_t e = int64_t(i) * n_frames + j;
      pt[e] = P + i;
      fr[e] = frame_no[j];
      ix[e] = pts2d_idx[int64_t(j) * n_pts + i];
    }
  Room room(h, m, n_pts, 0);
  room.put(h->X() + 3 * size_t(P), pts3d, int64_t(n_pts) * 3);
  room.put(h->ob_pt() + N, pt.data(), m);
  room.put(h->ob_frame() + N, fr.data(), m);
  room.put(h->ob_idx() + N, ix.data(), m);
  room.fill(h->ob_mm() + N, 1, m);
  // views = the frame count, ages 0, in _pts3DIdx (CMap.cpp:36-78)
  room.fill(h->pt_time() + P, 0, n_pts);
  room.fill(h->pt_kf() + P, 0, n_pts);
  room.fill(h->pt_views() + P, 0, n_pts);
  room.fill(h->pt_live() + P, 1, n_pts);
  if (room.rc) return room.rc;
  if (n_frames) k_fill_i32<<<grid(n_pts), 256, 0, h->s>>>(n_pts, h->pt_views() + P, n_frames);
  if (int rc = sync(h)) return rc;
  h->obs.commit(m);
  h->pts.commit(n_pts);
  h->live_h.resize(size_t(P) + n_pts, 1);
  h->n_live += n_pts;
  if (pts3d_idx)
    for (int32_t i = 0; i < n_pts; ++i) pts3d_idx[i] = P + i;
  h->ocsr = h->dcsr = false;
  return 0;
}

int sfm_map_add_point_matches(sfm_map* h, int32_t n, const int32_t* pts3d_idx, const int32_t* pts2d_idx,
                              int32_t frame_no) {
  if (const auto [rc, go] = open_list(h, n, pts3d_idx, pts3d_idx && pts2d_idx, true); !go) return rc;
  const std::vector<int32_t> fr(size_t(n), frame_no);
  const int64_t N = h->obs.n();
  Room room(h, n, 0, 0);
  room.put(h->ob_pt() + N, pts3d_idx, n);
  room.put(h->ob_frame() + N, fr.data(), n);
  room.put(h->ob_idx() + N, pts2d_idx, n);
  room.fill(h->ob_mm() + N, 1, n);
  if (room.rc) return room.rc;
  k_add_views<<<grid(n), 256, 0, h->s>>>(n, h->ob_pt() + N, h->pt_views());  // _ptsViews[idx]++
  if (int rc = sync(h)) return rc;
  h->obs.commit(n);
  h->ocsr = false;
  return 0;
}

int sfm_map_add_descriptors(sfm_map* h, int32_t n, const int32_t* pts3d_idx, const uint8_t* desc) {
  if (const auto [rc, go] = open_list(h, n, pts3d_idx, pts3d_idx && desc, true); !go) return rc;
  // rows are desc_bytes = 8 W bytes: copy as words (unaligned host bytes)
  std::vector<uint64_t> words(size_t(n) * h->W);
  std::memcpy(words.data(), desc, words.size() * sizeof(uint64_t));
  const int64_t R = h->rows.n();
  Room room(h, 0, 0, n);
  room.put(h->desc() + size_t(R) * h->W, words.data(), int64_t(n) * h->W);
  room.put(h->desc_pt() + R, pts3d_idx, n);
  if (room.rc) return room.rc;
  if (int rc = sync(h)) return rc;
  h->rows.commit(n);
  h->dcsr = false;
  return 0;
}

// addPointMatches(pts3d_idx, rows, frame_no) (with_observations != 0) then
// addDescriptors(pts3d_idx, descriptor rows `rows` of the matcher's keyframe
// `slot`): the two lists go up once, the descriptor words are copied from the
// matcher's keyframe store on the device, one synchronisation.
int sfm_map_add_keyframe_rows(sfm_map* h, sfm_matcher* mt, int32_t slot, int32_t frame_no, int32_t n,
                              const int32_t* pts3d_idx, const int32_t* rows, int32_t with_observations) {
  SFM_TRACE("sfm_map_add_keyframe_rows");
  if (!h || !mt) return mapfail(SFM_EINVAL, "NULL handle");
  if (n < 0) return mapfail(SFM_EINVAL, "negative size");
  if (n && (!pts3d_idx || !rows)) return mapfail(SFM_EINVAL, "NULL argument");
  if (matcher_words(mt) != h->W || matcher_device(mt) != h->device)
    return mapfail(SFM_EINVAL, "the map and the matcher differ in descriptor width or device");
  if (int rc = check_pts(h, n, pts3d_idx, true)) return rc;
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  const uint64_t* kdesc = nullptr;
  int kn = 0;
  hipEvent_t ready = nullptr;
  if (int rc = matcher_keyframe_rows(mt, slot, &kdesc, &kn, &ready)) return rc;
  for (int32_t i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= kn)
      return mapfail(SFM_EINVAL, "keyframe row " + std::to_string(rows[i]) + " out of range at " + std::to_string(i));
  if (n == 0) return 0;
  int rc = 0;
  auto* up = scratch<int32_t>(h, "kfrows", 2 * size_t(n), &rc);
  int32_t* pin = pin_reserve(h, 2 * size_t(n), &rc);
  if (rc) return rc;
  const Room room(h, with_observations ? n : 0, 0, n);  // (written on the device below, not through put / fill)
  if (room.rc) return room.rc;
  const int64_t N = h->obs.n(), R = h->rows.n();
  // the keyframe's rows are the matcher's upload: ordered after its stream
  if (hipStreamWaitEvent(h->s, ready, 0) != hipSuccess) return mapfail(SFM_EIO, "stream wait failed");
  (void)hipStreamSynchronize(h->s);  // (the pinned block may feed an earlier copy)
  std::memcpy(pin, pts3d_idx, sizeof(int32_t) * size_t(n));
  std::memcpy(pin + n, rows, sizeof(int32_t) * size_t(n));
  (void)hipMemcpyAsync(up, pin, sizeof(int32_t) * 2 * size_t(n), hipMemcpyHostToDevice, h->s);
  const size_t nb = sizeof(int32_t) * size_t(n);
  if (with_observations) {
    (void)hipMemcpyAsync(h->ob_pt() + N, up, nb, hipMemcpyDeviceToDevice, h->s);
    (void)hipMemcpyAsync(h->ob_idx() + N, up + n, nb, hipMemcpyDeviceToDevice, h->s);
    k_fill_i32<<<grid(n), 256, 0, h->s>>>(n, h->ob_frame() + N, frame_no);
    (void)hipMemsetAsync(h->ob_mm() + N, 1, size_t(n), h->s);
    k_add_views<<<grid(n), 256, 0, h->s>>>(n, up, h->pt_views());  // _ptsViews[idx]++
  }
  launch_copy_desc_rows(h->s, n, up + n, kdesc, h->W, h->desc() + size_t(R) * h->W);
  (void)hipMemcpyAsync(h->desc_pt() + R, up, nb, hipMemcpyDeviceToDevice, h->s);
  if ((rc = sync(h))) return rc;
  if (with_observations) {
    h->obs.commit(n);
    h->ocsr = false;
  }
  h->rows.commit(n);
  h->dcsr = false;
  return 0;
}

int sfm_map_get_points(sfm_map* h, int32_t n, const int32_t* pts3d_idx, double* pts3d) {
  SFM_TRACE("sfm_map_get_points");
  if (const auto [rc, go] = open_list(h, n, pts3d_idx, pts3d_idx && pts3d, false); !go) return rc;
  // gathered on the device: the indices up, n points down (the whole X
  // array went down before: 140 KB per tracked frame at 6k points)
  int rc = 0;
  auto* di = scratch<int32_t>(h, "gi", size_t(n), &rc);
  auto* dv = scratch<double>(h, "gv", 3 * size_t(n), &rc);
  pin_reserve(h, 8 * size_t(n) + 8, &rc);
  if (rc) return rc;
  (void)hipStreamSynchronize(h->s);  // (the pinned block may feed an earlier copy)
  std::memcpy(h->pin, pts3d_idx, sizeof(int32_t) * size_t(n));
  double* pv = reinterpret_cast<double*>(h->pin + ((size_t(n) + 1) & ~size_t(1)));
  (void)hipMemcpyAsync(di, h->pin, sizeof(int32_t) * size_t(n), hipMemcpyHostToDevice, h->s);
  k_gather_points<<<grid(n), 256, 0, h->s>>>(n, di, h->X(), dv);
  if (hipMemcpyAsync(pv, dv, sizeof(double) * 3 * size_t(n), hipMemcpyDeviceToHost, h->s) != hipSuccess)
    return mapfail(SFM_EIO, "download failed");
  if (int r = sync(h)) return r;
  std::memcpy(pts3d, pv, sizeof(double) * 3 * size_t(n));
  return 0;
}

int sfm_map_set_points(sfm_map* h, int32_t n, const int32_t* pts3d_idx, const double* pts3d) {
  if (const auto [rc, go] = open_list(h, n, pts3d_idx, pts3d_idx && pts3d, false); !go) return rc;
  int rc = 0;
  auto* di = scratch<int32_t>(h, "si", size_t(n), &rc);
  auto* dv = scratch<double>(h, "sv", 3 * size_t(n), &rc);
  if (rc) return rc;
  if (hipMemcpyAsync(di, pts3d_idx, sizeof(int32_t) * size_t(n), hipMemcpyHostToDevice, h->s) != hipSuccess ||
      hipMemcpyAsync(dv, pts3d, sizeof(double) * 3 * size_t(n), hipMemcpyHostToDevice, h->s) != hipSuccess)
    return mapfail(SFM_EIO, "upload failed");
  k_scatter_points<<<grid(n), 256, 0, h->s>>>(n, di, dv, h->X());  // (indices expected unique)
  return sync(h);
}

int sfm_map_points_in_frames(sfm_map* h, int32_t n_frames, const int32_t* frame_no, int32_t capacity,
                             int32_t* pts3d_idx, int32_t* n_out) {
  if (!h || !n_out) return mapfail(SFM_EINVAL, "NULL argument");
  *n_out = 0;
  if (n_frames < 0) return mapfail(SFM_EINVAL, "negative size");
  if (n_frames == 0 || h->n_pts() == 0 || h->obs.n() == 0) return 0;
  if (!frame_no) return mapfail(SFM_EINVAL, "NULL frame list");
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  int rc = 0;
  const std::set<int32_t> distinct(frame_no, frame_no + n_frames);  // ascending
  const std::vector<int32_t> fs(distinct.begin(), distinct.end());
  auto* fset = scratch<int32_t>(h, "fset", fs.size(), &rc);
  auto* out = scratch<int32_t>(h, "pout", size_t(h->n_pts()), &rc);
  auto* dn = scratch<int32_t>(h, "pn", 1, &rc);
  if (rc) return rc;
  (void)hipMemcpyAsync(fset, fs.data(), sizeof(int32_t) * fs.size(), hipMemcpyHostToDevice, h->s);
  if ((rc = select_points_in_frames(h, fset, int(fs.size()), nullptr, 0, out, dn))) return rc;
  int32_t n = 0;
  (void)hipMemcpyAsync(&n, dn, sizeof(int32_t), hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  *n_out = n;
  if (n > capacity) return mapfail(SFM_EINVAL, "capacity " + std::to_string(capacity) + " < " + std::to_string(n));
  if (n && (!pts3d_idx || hipMemcpy(pts3d_idx, out, sizeof(int32_t) * size_t(n), hipMemcpyDeviceToHost) != hipSuccess))
    return mapfail(SFM_EIO, "download failed");
  return 0;
}

int sfm_map_points_in_frame(sfm_map* h, int32_t frame_no, int32_t capacity, int32_t* pts3d_idx, int32_t* n3_out,
                            int32_t* pts2d_idx, int32_t* n2_out) {
  if (!h || !n3_out || !n2_out) return mapfail(SFM_EINVAL, "NULL argument");
  *n3_out = *n2_out = 0;
  const int64_t N = h->obs.n();
  if (N == 0) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  int rc = 0;
  if (int r = ensure_ocsr(h)) return r;
  auto* flag = scratch<uint8_t>(h, "fflag", size_t(N), &rc);
  auto* sel = scratch<int32_t>(h, "fsel", size_t(N), &rc);
  auto* dn = scratch<int32_t>(h, "fn", 1, &rc);
  if (rc) return rc;
  k_flag_frame<<<grid(N), 256, 0, h->s>>>(N, h->ob_frame(), h->ob_mm(), frame_no, flag);
  if (int r = select_flagged(h, "fselt", flag, sel, dn, int(N))) return r;
  int32_t n = 0;
  (void)hipMemcpyAsync(&n, dn, sizeof(int32_t), hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  if (n == 0) return 0;
  auto* cnt = scratch<int32_t>(h, "fcnt", size_t(n), &rc);
  auto* off2 = scratch<int32_t>(h, "foff", size_t(n), &rc);
  auto* out3 = scratch<int32_t>(h, "fo3", size_t(n), &rc);
  if (rc) return rc;
  k_dup_count<<<grid(n), 256, 0, h->s>>>(n, sel, h->ob_pt(), h->ob_frame(), h->orow, h->ooff, frame_no, cnt);
  if (int r = exclusive_sum(h, "fscan", cnt, off2, n)) return r;
  int32_t last[2] = {0, 0};
  (void)hipMemcpyAsync(last, off2 + n - 1, sizeof(int32_t), hipMemcpyDeviceToHost, h->s);
  (void)hipMemcpyAsync(last + 1, cnt + n - 1, sizeof(int32_t), hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  const int32_t n2 = last[0] + last[1];
  auto* out2 = scratch<int32_t>(h, "fo2", size_t(std::max(n2, 1)), &rc);
  if (rc) return rc;
  k_dup_fill<<<grid(n), 256, 0, h->s>>>(n, sel, h->ob_pt(), h->ob_frame(), h->ob_idx(), h->orow, h->ooff, frame_no,
                                        off2, out3, out2);
  if (int r = sync(h)) return r;
  *n3_out = n;
  *n2_out = n2;
  if (n > capacity || n2 > capacity)
    return mapfail(SFM_EINVAL, "capacity " + std::to_string(capacity) + " < " + std::to_string(std::max(n, n2)));
  if (!pts3d_idx || !pts2d_idx) return mapfail(SFM_EINVAL, "NULL output");
  if (hipMemcpy(pts3d_idx, out3, sizeof(int32_t) * size_t(n), hipMemcpyDeviceToHost) != hipSuccess ||
      (n2 && hipMemcpy(pts2d_idx, out2, sizeof(int32_t) * size_t(n2), hipMemcpyDeviceToHost) != hipSuccess))
    return mapfail(SFM_EIO, "download failed");
  return 0;
}

int sfm_map_points_in_frame_multi(sfm_map* h, int32_t n_frames, const int32_t* frame_no, int64_t capacity,
                                  int32_t* pts3d_idx, int32_t* off3, int32_t* pts2d_idx, int32_t* off2) {
  SFM_TRACE("sfm_map_points_in_frame_multi");
  if (!h || !off3 || !off2 || (n_frames > 0 && !frame_no)) return mapfail(SFM_EINVAL, "NULL argument");
  if (n_frames < 0) return mapfail(SFM_EINVAL, "negative size");
  for (int i = 0; i <= n_frames; ++i) off3[i] = off2[i] = 0;
  const int64_t N = h->obs.n();
  if (N == 0 || n_frames == 0) return 0;
  std::vector<int2> fr(static_cast<size_t>(n_frames));
  for (int i = 0; i < n_frames; ++i) fr[i] = make_int2(frame_no[i], i);
  std::sort(fr.begin(), fr.end(), [](int2 a, int2 b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
  for (int i = 1; i < n_frames; ++i)
    if (fr[i].x == fr[i - 1].x) return mapfail(SFM_EINVAL, "frame " + std::to_string(fr[i].x) + " queried twice");
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  int rc = 0;
  if (int r = ensure_ocsr(h)) return r;
  // every observation keyed by its frame's position in the query list; a
  // stable sort groups them frame by frame, each frame's in emplace order
  // (its equal_range)
  auto* dfr = scratch<int2>(h, "mfr", size_t(n_frames), &rc);
  auto* key = scratch<uint32_t>(h, "mk", size_t(N), &rc);
  auto* key2 = scratch<uint32_t>(h, "mk2", size_t(N), &rc);
  auto* iv = scratch<int32_t>(h, "mi", size_t(N), &rc);
  auto* sel = scratch<int32_t>(h, "msel", size_t(N), &rc);
  auto* fcnt = scratch<int32_t>(h, "mfc", size_t(n_frames) + 1, &rc);
  if (rc) return rc;
  (void)hipMemcpyAsync(dfr, fr.data(), sizeof(int2) * fr.size(), hipMemcpyHostToDevice, h->s);
  (void)hipMemsetAsync(fcnt, 0, sizeof(int32_t) * (size_t(n_frames) + 1), h->s);
  k_frame_rank<<<grid(N), 256, 0, h->s>>>(N, h->ob_frame(), h->ob_mm(), dfr, n_frames, key, iv);
  k_count_keys<<<grid(N), 256, 0, h->s>>>(N, reinterpret_cast<const int32_t*>(key), fcnt);
  int bits = 1;
  while ((1 << bits) <= n_frames) ++bits;
  if (int r = sort_pairs(h, "msort", key, key2, iv, sel, int(N), bits, "sort failed")) return r;
  // per sorted entry: how many 2D indices its point has in the entry's frame
  // (0 past the queried frames), their exclusive scan, then the frames'
  // offsets on the device: one readback of 2 (nf + 1) ints
  auto* cnt = scratch<int32_t>(h, "mcnt", size_t(N), &rc);
  auto* eoff = scratch<int32_t>(h, "moff", size_t(N), &rc);
  auto* offs = scratch<int32_t>(h, "moffs", 2 * (size_t(n_frames) + 1), &rc);
  if (rc) return rc;
  k_dup_count_ranked<<<grid(N), 256, 0, h->s>>>(N, sel, key2, n_frames, h->ob_pt(), h->ob_frame(), h->orow, h->ooff,
                                                 cnt);
  if (int r = exclusive_sum(h, "mscan", cnt, eoff, int(N))) return r;
  k_frame_offsets<<<1, 1, 0, h->s>>>(n_frames, fcnt, N, cnt, eoff, offs);
  // (readbacks through the pinned block: a pageable copy is staged by the
  // runtime, ~2x the time at these sizes)
  int32_t* offs_h = pin_reserve(h, 2 * (size_t(n_frames) + 1), &rc);
  if (rc) return rc;
  (void)hipMemcpyAsync(offs_h, offs, sizeof(int32_t) * 2 * (size_t(n_frames) + 1), hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  for (int i = 0; i <= n_frames; ++i) {
    off3[i] = offs_h[i];
    off2[i] = offs_h[n_frames + 1 + i];
  }
  const int32_t n = off3[n_frames], n2 = off2[n_frames];
  if (n == 0) return 0;
  if (int64_t(n) > capacity || int64_t(n2) > capacity)
    return mapfail(SFM_EINVAL, "capacity " + std::to_string(capacity) + " < " + std::to_string(std::max(n, n2)));
  if (!pts3d_idx || !pts2d_idx) return mapfail(SFM_EINVAL, "NULL output");
  auto* out3 = scratch<int32_t>(h, "mo3", size_t(n), &rc);
  auto* out2 = scratch<int32_t>(h, "mo2", size_t(std::max(n2, 1)), &rc);
  if (rc) return rc;
  k_dup_fill<<<grid(n), 256, 0, h->s>>>(n, sel, h->ob_pt(), h->ob_frame(), h->ob_idx(), h->orow, h->ooff, INT32_MIN,
                                        eoff, out3, out2);
  int32_t* ph = pin_reserve(h, size_t(n) + size_t(n2), &rc);
  if (rc) return rc;
  (void)hipMemcpyAsync(ph, out3, sizeof(int32_t) * size_t(n), hipMemcpyDeviceToHost, h->s);
  if (n2) (void)hipMemcpyAsync(ph + n, out2, sizeof(int32_t) * size_t(n2), hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  std::memcpy(pts3d_idx, ph, sizeof(int32_t) * size_t(n));
  if (n2) std::memcpy(pts2d_idx, ph + n, sizeof(int32_t) * size_t(n2));
  return 0;
}

int sfm_map_representative_descriptors(sfm_map* h, int32_t n, const int32_t* pts3d_idx, uint8_t* desc_out,
                                       int32_t* best_row) {
  if (const auto [rc, go] = open_list(h, n, pts3d_idx, pts3d_idx && desc_out, true); !go) return rc;
  int rc = 0;
  if (int r = ensure_dcsr(h)) return r;
  // every queried point needs a row (the reference reads row -1 otherwise)
  std::vector<int32_t> off(size_t(h->n_pts()) + 1);
  (void)hipMemcpyAsync(off.data(), h->doff, sizeof(int32_t) * off.size(), hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  for (int32_t i = 0; i < n; ++i)
    if (off[size_t(pts3d_idx[i]) + 1] == off[size_t(pts3d_idx[i])])
      return mapfail(SFM_EINVAL, "point " + std::to_string(pts3d_idx[i]) + " has no descriptor row");
  auto* q = scratch<int32_t>(h, "rq", size_t(n), &rc);
  auto* best = scratch<int32_t>(h, "rb", size_t(n), &rc);
  auto* out = scratch<uint64_t>(h, "ro", size_t(n) * h->W, &rc);
  if (rc) return rc;
  (void)hipMemcpyAsync(q, pts3d_idx, sizeof(int32_t) * size_t(n), hipMemcpyHostToDevice, h->s);
  if (int r = launch_map_repr(h, n, q, nullptr, best, out)) return r;
  (void)hipMemcpyAsync(desc_out, out, size_t(n) * h->W * sizeof(uint64_t), hipMemcpyDeviceToHost, h->s);
  std::vector<int32_t> b(static_cast<size_t>(n));
  (void)hipMemcpyAsync(b.data(), best, sizeof(int32_t) * size_t(n), hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  if (best_row) std::memcpy(best_row, b.data(), sizeof(int32_t) * size_t(n));
  return 0;
}

// CSfM::findMapPointsInCurrentFrame (CSfM.cpp:634-692) in one call: the
// points of the keyframes (getPointsInFrames), minus the frame's matched
// points, projected with the frame's pose, their representative descriptors,
// matched in the (min, max) window against the current frame's unmatched
// keypoints, which the matcher holds (sfm_matcher_push_frame).  Everything
// stays on the device: one readback of the query count, one of the results
// (the composed calls downloaded every map point and the descriptors, and
// uploaded them again for the match: ~10 synchronisations per frame).
int sfm_map_match_frame(sfm_map* h, sfm_matcher* mt, int32_t n_frames, const int32_t* frame_no, int32_t n_existing,
                        const int32_t* existing_pts, const double* R9, const double* t3, const double* K9,
                        int32_t n_train, const int32_t* train_idx, double ratio_test, double min_distance,
                        double max_distance, int32_t capacity, int32_t* pts3d_match, int32_t* train_match,
                        int32_t* n_matches) {
  SFM_TRACE("sfm_map_match_frame");
  if (!h || !mt || !n_matches) return mapfail(SFM_EINVAL, "NULL handle");
  *n_matches = 0;
  if (n_frames < 0 || n_existing < 0 || n_train < 0) return mapfail(SFM_EINVAL, "negative size");
  if ((n_frames && !frame_no) || (n_existing && !existing_pts) || (n_train && !train_idx) || !R9 || !t3 || !K9)
    return mapfail(SFM_EINVAL, "NULL argument");
  if (matcher_words(mt) != h->W || matcher_device(mt) != h->device)
    return mapfail(SFM_EINVAL, "the map and the matcher differ in descriptor width or device");
  if (int rc = check_pts(h, n_existing, existing_pts, true)) return rc;
  const int n_cur = matcher_current_n(mt);
  if (n_cur < 0) return mapfail(SFM_EINVAL, "push the current frame to the matcher first");
  for (int i = 0; i < n_train; ++i)
    if (train_idx[i] < 0 || train_idx[i] >= n_cur) return mapfail(SFM_EINVAL, "train index out of range");
  if (n_frames == 0 || h->n_pts() == 0 || h->obs.n() == 0 || n_train < 2) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  int rc = 0;
  const int P = h->n_pts();
  const std::set<int32_t> distinct(frame_no, frame_no + n_frames);  // ascending
  const std::vector<int32_t> fs(distinct.begin(), distinct.end());
  if (int r = ensure_dcsr(h)) return r;
  const size_t n_up = fs.size() + size_t(n_existing) + size_t(n_train);
  auto* fset = scratch<int32_t>(h, "fset", n_up, &rc);
  // the selected points, then (after k_map_repr) their representative rows:
  // one download for both
  auto* out = scratch<int32_t>(h, "pout", 2 * size_t(P), &rc);
  auto* dn = scratch<int32_t>(h, "pn", 1, &rc);
  auto* qd = scratch<uint64_t>(h, "mq", size_t(P) * h->W, &rc);
  auto* uv = scratch<double>(h, "muv", 2 * size_t(P), &rc);
  pin_reserve(h, std::max(2 * size_t(P) + 1, n_up), &rc);
  if (rc) return rc;
  if (h->ev.create(hipEventDisableTiming) != hipSuccess) return mapfail(SFM_EIO, "hipEventCreate failed");
  // frames, the frame's matched points and the train subset in one upload
  (void)hipStreamSynchronize(h->s);  // (the pinned block may feed an earlier copy)
  std::memcpy(h->pin, fs.data(), sizeof(int32_t) * fs.size());
  if (n_existing) std::memcpy(h->pin + fs.size(), existing_pts, sizeof(int32_t) * size_t(n_existing));
  std::memcpy(h->pin + fs.size() + n_existing, train_idx, sizeof(int32_t) * size_t(n_train));
  (void)hipMemcpyAsync(fset, h->pin, sizeof(int32_t) * n_up, hipMemcpyHostToDevice, h->s);
  if ((rc = select_points_in_frames(h, fset, int(fs.size()), fset + fs.size(), n_existing, out, dn))) return rc;
  // no readback of the count here: the kernels below run on its bound P and
  // read the count itself (k_map_repr, k_project, the matcher's acceptance)
  int32_t* best = out + P;
  if (int r = launch_map_repr(h, P, out, dn, best, qd)) return r;
  k_project<<<grid(P), 256, 0, h->s>>>(P, dn, out, h->X(), R9[0], R9[1], R9[2], R9[3], R9[4], R9[5], R9[6], R9[7],
                                       R9[8], t3[0], t3[1], t3[2], K9[0], K9[4], K9[2], K9[5], uv);
  // points, representative rows and the count in one download
  (void)hipMemcpyAsync(h->pin, out, sizeof(int32_t) * 2 * size_t(P), hipMemcpyDeviceToHost, h->s);
  (void)hipMemcpyAsync(h->pin + 2 * size_t(P), dn, sizeof(int32_t), hipMemcpyDeviceToHost, h->s);
  if (hipEventRecord(h->ev, h->s) != hipSuccess) return mapfail(SFM_EIO, "hipEventRecord failed");
  int* res = nullptr;
  if ((rc = matcher_match_current_dev(mt, h->ev, qd, uv, P, dn, fset + fs.size() + n_existing, n_train, ratio_test,
                                      min_distance, max_distance, &res)))
    return rc;
  if (int r = sync(h)) return r;
  const int n_new = h->pin[2 * size_t(P)];
  for (int i = 0; i < n_new; ++i)
    if (h->pin[P + i] < 0)
      return mapfail(SFM_EINVAL, "point " + std::to_string(h->pin[i]) + " has no descriptor row");
  const int m = res[2 * P];
  if (m > capacity) return mapfail(SFM_EINVAL, "capacity " + std::to_string(capacity) + " < " + std::to_string(m));
  for (int k = 0; k < m; ++k) {
    pts3d_match[k] = h->pin[res[k]];
    train_match[k] = train_idx[res[P + k]];
  }
  *n_matches = m;
  return 0;
}

// ---- culling: CMap.cpp:384-574 and CSfM::cullKeyFrames.  Every call makes
// one host synchronisation (sfm_map_n_live none), besides buffer growth and
// a stale CSR's rebuild, which enqueue only.

int sfm_map_update_point_views(sfm_map* h, int32_t n, const int32_t* pts3d_idx) {
  if (const auto [rc, go] = open_list(h, n, pts3d_idx, pts3d_idx != nullptr, true); !go) return rc;
  int rc = 0;
  auto* di = scratch<int32_t>(h, "vi", size_t(n), &rc);
  if (rc) return rc;
  if (hipMemcpyAsync(di, pts3d_idx, sizeof(int32_t) * size_t(n), hipMemcpyHostToDevice, h->s) != hipSuccess)
    return mapfail(SFM_EIO, "upload failed");
  k_add_views<<<grid(n), 256, 0, h->s>>>(n, di, h->pt_views());
  return sync(h);
}

int sfm_map_increment_age(sfm_map* h, int32_t t_inc, int32_t kf_inc) {
  if (!h) return mapfail(SFM_EINVAL, "NULL handle");
  if (h->n_pts() == 0) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  k_age<<<grid(h->n_pts()), 256, 0, h->s>>>(h->n_pts(), h->pt_live(), h->pt_time(), h->pt_kf(), t_inc, kf_inc);
  return sync(h);
}

int sfm_map_n_live(sfm_map* h, int32_t* n) {
  if (!h || !n) return mapfail(SFM_EINVAL, "NULL argument");
  *n = h->n_live;
  return 0;
}

int sfm_map_point_state(sfm_map* h, int32_t n, const int32_t* pts3d_idx, int32_t* out) {
  if (const auto [rc, go] = open_list(h, n, pts3d_idx, pts3d_idx && out, false); !go) return rc;
  if (int rc = ensure_csrs(h)) return rc;
  int rc = 0;
  auto* di = scratch<int32_t>(h, "vi", size_t(n), &rc);
  auto* dout = scratch<int32_t>(h, "vo", 5 * size_t(n), &rc);
  if (rc) return rc;
  if (hipMemcpyAsync(di, pts3d_idx, sizeof(int32_t) * size_t(n), hipMemcpyHostToDevice, h->s) != hipSuccess)
    return mapfail(SFM_EIO, "upload failed");
  k_point_state<<<grid(n), 256, 0, h->s>>>(n, di, h->pt_time(), h->pt_kf(), h->pt_views(), h->ooff, h->pt_live(),
                                           dout);
  if (hipMemcpyAsync(out, dout, sizeof(int32_t) * 5 * size_t(n), hipMemcpyDeviceToHost, h->s) != hipSuccess)
    return mapfail(SFM_EIO, "download failed");
  return sync(h);
}

int sfm_map_remove_points_threshold(sfm_map* h, int32_t kf_threshold, float track_threshold, int32_t capacity,
                                    int32_t* cull_idx, int32_t* n_cull, int32_t* status) {
  SFM_TRACE("sfm_map_remove_points_threshold");
  if (!h || !n_cull) return mapfail(SFM_EINVAL, "NULL argument");
  *n_cull = 0;
  if (capacity < 0 || kf_threshold < 0) return mapfail(SFM_EINVAL, "negative size or threshold");
  if (capacity && !cull_idx) return mapfail(SFM_EINVAL, "NULL output");
  const int P = h->n_pts();
  if (P == 0) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  if (int rc = ensure_csrs(h)) return rc;
  int rc = 0;
  const size_t nres = 3 + 2 * size_t(P);  // count, sizes after, the culled list, the status
  auto* res = scratch<int32_t>(h, "cres", nres, &rc);
  auto* flag = scratch<uint8_t>(h, "cflag", size_t(P), &rc);
  if (rc || (rc = select_flagged(h, "csel", flag, res + 3, res, P, false))) return rc;
  const Removal m(h, nres);
  if (m.rc) return m.rc;
  k_cull_flag<<<grid(P), 256, 0, h->s>>>(P, h->pt_live(), h->pt_time(), h->pt_kf(), h->pt_views(), h->ooff,
                                         kf_threshold, track_threshold, flag);
  if (int r = select_flagged(h, "csel", flag, res + 3, res, P)) return r;
  if (int r = kill_and_compact(h, m, flag, res, capacity, res)) return r;
  const int32_t* ph = m.pin;
  (void)hipMemcpyAsync(m.pin, res, sizeof(int32_t) * nres, hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  const int32_t n = ph[0];
  *n_cull = n;
  if (n > capacity)  // (the device saw the same comparison and removed nothing)
    return mapfail(SFM_EINVAL, "capacity " + std::to_string(capacity) + " < " + std::to_string(n));
  compact_done(h, ph + 1);
  for (int32_t i = 0; i < n; ++i) {
    cull_idx[i] = ph[3 + i];
    h->live_h[size_t(ph[3 + i])] = 0;
  }
  h->n_live -= n;
  if (status) std::memcpy(status, ph + 3 + P, sizeof(int32_t) * size_t(P));
  return 0;
}

int sfm_map_remove_points(sfm_map* h, int32_t n, const int32_t* pts3d_idx, int32_t* status) {
  if (!h) return mapfail(SFM_EINVAL, "NULL handle");
  if (n < 0) return mapfail(SFM_EINVAL, "negative size");
  if (n && !pts3d_idx) return mapfail(SFM_EINVAL, "NULL argument");
  if (int rc = check_pts(h, n, pts3d_idx, true)) return rc;
  for (int32_t i = 1; i < n; ++i)
    if (pts3d_idx[i] <= pts3d_idx[i - 1])
      return mapfail(SFM_EINVAL, "the list must be ascending and distinct (at " + std::to_string(i) + ")");
  const int P = h->n_pts();
  if (n == 0) {
    if (status && P) std::memset(status, 0, sizeof(int32_t) * size_t(P));
    return 0;
  }
  if (hipSetDevice(h->device) != hipSuccess) return mapfail(SFM_ENODEV, "hipSetDevice failed");
  int rc = 0;
  const size_t nres = 3 + 2 * size_t(P);
  auto* res = scratch<int32_t>(h, "cres", nres, &rc);
  auto* flag = scratch<uint8_t>(h, "cflag", size_t(P), &rc);
  auto* di = scratch<int32_t>(h, "vi", size_t(n), &rc);
  if (rc) return rc;
  const Removal m(h, nres);
  if (m.rc) return m.rc;
  if (hipMemcpyAsync(di, pts3d_idx, sizeof(int32_t) * size_t(n), hipMemcpyHostToDevice, h->s) != hipSuccess)
    return mapfail(SFM_EIO, "upload failed");
  (void)hipMemsetAsync(flag, 0, size_t(P), h->s);
  k_flag_list<<<grid(n), 256, 0, h->s>>>(n, di, flag);
  if (int r = kill_and_compact(h, m, flag, nullptr, 0, res)) return r;
  const int32_t* ph = m.pin;
  (void)hipMemcpyAsync(m.pin + 1, res + 1, sizeof(int32_t) * (nres - 1), hipMemcpyDeviceToHost, h->s);
  if (int r = sync(h)) return r;
  compact_done(h, ph + 1);
  for (int32_t i = 0; i < n; ++i) h->live_h[size_t(pts3d_idx[i])] = 0;
  h->n_live -= n;
  if (status) std::memcpy(status, ph + 3 + P, sizeof(int32_t) * size_t(P));
  return 0;
}

int sfm_map_remove_frame(sfm_map* h, int32_t frame_no, int32_t n, const int32_t* pts3d_idx) {
  if (n < 0) return mapfail(SFM_EINVAL, "negative size");
  const int32_t off[2] = {0, n};
  int32_t culled = 0;
  return walk_keyframes(h, 1, 1, &frame_no, off, pts3d_idx, 0, 0.0, &culled);
}

int sfm_map_points_seen_by_at_least(sfm_map* h, int32_t n, const int32_t* pts3d_idx, int32_t n_frames, double ratio,
                                    int32_t* result) {
  if (!result) return mapfail(SFM_EINVAL, "NULL argument");
  *result = 0;
  if (n < 0) return mapfail(SFM_EINVAL, "negative size");
  const int32_t off[2] = {0, n}, f = 0;
  return walk_keyframes(h, 2, 1, &f, off, pts3d_idx, n_frames, ratio, result);
}

int sfm_map_cull_keyframes(sfm_map* h, int32_t n_kf, const int32_t* frame_no, const int32_t* off, const int32_t* pts,
                           int32_t n_frames, double ratio, int32_t* culled) {
  SFM_TRACE("sfm_map_cull_keyframes");
  return walk_keyframes(h, 0, n_kf, frame_no, off, pts, n_frames, ratio, culled);
}

}  // extern "C"

namespace sfm {
// The device copy of the map's points for sfm_track_pnp, which reads it on
// the matcher's stream: the map stream is drained first (its calls already
// synchronise before returning; this keeps the rule local).
const double* map_points_dev(sfm_map* h, int32_t* n_pts, int* device) {
  (void)hipStreamSynchronize(h->s);
  *n_pts = h->n_pts();
  *device = h->device;
  return h->X();
}

// The points and live flags where they are (map_internal.h): no copy and no
// synchronisation; the reader orders its stream after `stream` with an event.
MapPointsView map_points_view(sfm_map* h) {
  return MapPointsView{h->X(), h->pt_live(), h->n_pts(), h->n_live, h->device, h->s};
}
}  // namespace sfm
