// Per-frame descriptor matcher for gfx950.
//
// Replaces brisk::BruteForceMatcher::knnMatch(k = 2) (called at
// /root/reference/CTracker.cpp:117, 214, 381, 433) and the reference's
// sequential acceptance loop, identical in all four matchFeatures overloads
// (CTracker.cpp:122-148, 221-249, 390-416, 441-467):
//
//   for i in queries (in order):
//     accept if d^2 > min^2 && d^2 < max^2 && float(d0)/float(d1) < ratio
//            && (train j0 unmatched || d0 < bestDist[j0])
//     new j0 -> append (i, j0); better -> overwrite the query at j0's slot
//
// Order-free form: for each train j the surviving query is the
// FIRST accepted query with the minimum distance, and the output slots are
// ordered by the first accepted query of each j -- integer min-reductions
// (atomicMin on packed keys), bit-exact and independent of scheduling.  2-NN
// ties go to the lower train index (the restated knnMatch convention): the
// search keeps the two smallest (distance << 32 | train) keys, so the scan
// order of the train rows does not matter and the rows can be split across
// workgroups and waves.
//
// Hot-path layout: an sfm_matcher handle keeps the last two frames'
// keypoints and descriptors resident in HBM (one upload per frame, the
// _prevFrame = _currFrame swap of CSfM.cpp:626-629), pools every device and
// pinned buffer (no allocation per call) and runs a call as one stream of
// launches with one host sync.  The 2-NN search is a 2-D grid (64 queries x
// a train slice per workgroup, four waves each scanning a quarter of the
// slice), so a 2k x 2k frame pair fills the chip; train rows are
// wave-uniform 64-B scalar loads, the query lives in VGPRs.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <map>
#include <string>
#include <vector>
#include "sfm_trace.h"
#include "../../include/sfm_amd.h"
#include "ordered_compact.h"
#include "frame_internal.h"
#include "mappoint_internal.h"
#include "dev_mem.h"

using sfm::DevArr;
using sfm::DevBuf;
using sfm::Event;
using sfm::PinBuf;
using sfm::Stream;

namespace {

constexpr int kQ = 64;       // queries per workgroup (one per lane)
constexpr int kWaves = 4;    // waves per workgroup, each a quarter of the train slice
constexpr unsigned long long kNoKey = ~0ull;

// branch-free: two compares and three selects per candidate
__device__ __forceinline__ void top2_insert(unsigned long long k, unsigned long long& k0, unsigned long long& k1) {
  const bool lt0 = k < k0, lt1 = k < k1;
  k1 = lt0 ? k0 : (lt1 ? k : k1);
  k0 = lt0 ? k : k0;
}

// Partial 2-NN of query block qb against train slice sl (one workgroup).
// Query i is row qidx[i] of q (qidx == nullptr: row i), train t is row
// tidx[t] of tr; part[(sl * n0 + i) * 2 + {0,1}] = the two smallest keys.
template <int W, bool kIdx>
__device__ __forceinline__ void knn2_block(const uint64_t* __restrict__ q, const int* __restrict__ qidx, int n0,
                                           const uint64_t* __restrict__ tr, const int* __restrict__ tidx, int n1,
                                           int slice, unsigned long long* __restrict__ part, int qb, int sl) {
  __shared__ unsigned long long red[kWaves][kQ][2];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: the train loop is scalar
  const int i = qb * kQ + lane;
  uint64_t x[W];
  if (i < n0) {
    const size_t row = qidx ? size_t(qidx[i]) : size_t(i);
#pragma unroll
    for (int k = 0; k < W; ++k) x[k] = q[row * W + k];
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) x[k] = 0ull;
  }
  unsigned long long k0 = kNoKey, k1 = kNoKey;
  const int t0 = sl * slice, t1 = min(n1, t0 + slice);
  const int per = (t1 - t0 + kWaves - 1) / kWaves;
  const int a = t0 + w * per, b = min(t1, a + per);
  // four rows in flight per step (four 64-B scalar loads, then the
  // popcounts), then the remainder
  int t = a;
  for (; t + 4 <= b; t += 4) {
    const uint64_t* r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = tr + (kIdx ? size_t(tidx[t + u]) : size_t(t + u)) * W;
    uint64_t y[4][W];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < W; ++k) y[u][k] = r[u][k];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      unsigned d = 0;
#pragma unroll
      for (int k = 0; k < W; ++k) d += unsigned(__popcll(x[k] ^ y[u][k]));
      top2_insert((static_cast<unsigned long long>(d) << 32) | unsigned(t + u), k0, k1);
    }
  }
  for (; t < b; ++t) {
    const uint64_t* r = tr + (kIdx ? size_t(tidx[t]) : size_t(t)) * W;   // wave-uniform: scalar loads
    unsigned d = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) d += unsigned(__popcll(x[k] ^ r[k]));
    top2_insert((static_cast<unsigned long long>(d) << 32) | unsigned(t), k0, k1);
  }
  red[w][lane][0] = k0;
  red[w][lane][1] = k1;
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int v = 1; v < kWaves; ++v) {
      top2_insert(red[v][lane][0], k0, k1);
      top2_insert(red[v][lane][1], k0, k1);
    }
    if (i < n0) {
      part[(size_t(sl) * n0 + i) * 2] = k0;
      part[(size_t(sl) * n0 + i) * 2 + 1] = k1;
    }
  }
}

// query block blockIdx.x against train slice blockIdx.y
template <int W, bool kIdx>
__global__ __launch_bounds__(kQ * kWaves) void k_knn2_part(const uint64_t* __restrict__ q, const int* __restrict__ qidx,
                                                           int n0, const uint64_t* __restrict__ tr,
                                                           const int* __restrict__ tidx, int n1, int slice,
                                                           unsigned long long* __restrict__ part) {
  knn2_block<W, kIdx>(q, qidx, n0, tr, tidx, n1, slice, part, blockIdx.x, blockIdx.y);
}

// The same for every item of a point-creation call (pair_points_run): item
// blockIdx.z's query rows against the common train rows.  The grid's x is
// sized for the longest item; a workgroup past its own item's rows leaves as
// a whole, before the LDS and the barrier.
template <int W>
__global__ __launch_bounds__(kQ * kWaves) void k_knn2_part_items(const sfm::PairItem* __restrict__ items,
                                                                 const int* __restrict__ idx,
                                                                 const uint64_t* __restrict__ tr,
                                                                 const int* __restrict__ tidx, int n1, int slice,
                                                                 unsigned long long* __restrict__ part) {
  const sfm::PairItem& it = items[blockIdx.z];
  const int n0 = it.n0;
  if (int(blockIdx.x) * kQ >= n0) return;
  knn2_block<W, true>(it.desc, idx + it.idx_off, n0, tr, tidx, n1, slice, part + it.part_off, blockIdx.x, blockIdx.y);
}

__device__ __forceinline__ void merge_parts(const unsigned long long* __restrict__ part, int n0, int nslice, int i,
                                            unsigned long long& k0, unsigned long long& k1) {
  k0 = kNoKey;
  k1 = kNoKey;
  for (int s = 0; s < nslice; ++s) {
    top2_insert(part[(size_t(s) * n0 + i) * 2], k0, k1);
    top2_insert(part[(size_t(s) * n0 + i) * 2 + 1], k0, k1);
  }
}

// The 2-NN result alone (sfm_knn2_hamming): best / second train + distance.
__global__ void k_knn2_merge(const unsigned long long* __restrict__ part, int n0, int nslice, int* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n0) return;
  unsigned long long k0, k1;
  merge_parts(part, n0, nslice, i, k0, k1);
  out[i] = k0 == kNoKey ? -1 : int(k0 & 0xffffffffu);
  out[n0 + i] = k0 == kNoKey ? (1 << 30) : int(k0 >> 32);
  out[2 * n0 + i] = k1 == kNoKey ? -1 : int(k1 & 0xffffffffu);
  out[3 * n0 + i] = k1 == kNoKey ? (1 << 30) : int(k1 >> 32);
}

// Merge + the acceptance test of query i + the per-train min-reductions:
//   key[j]   = min over accepted queries of (d0 << 32 | i)  -> surviving query
//   first[j] = min over accepted queries of i               -> slot order
// Positions are those of rows qidx[i] / tidx[j] (nullptr: i / j).
// (n0_dev: the query count on the device, n0 its bound -- sfm_map_match_frame)
__device__ __forceinline__ void accept_query(const unsigned long long* __restrict__ part, int n0, int nslice, int i,
                                             const double* __restrict__ p0, const int* __restrict__ qidx,
                                             const double* __restrict__ p1, const int* __restrict__ tidx,
                                             double ratio_test, double minSq, double maxSq,
                                             unsigned long long* __restrict__ key, int* __restrict__ first) {
#pragma clang fp contract(off)
  unsigned long long k0, k1;
  merge_parts(part, n0, nslice, i, k0, k1);
  if (k0 == kNoKey || k1 == kNoKey) return;  // < 2 train rows: the reference reads past matches[i] (UB)
  const int j = int(k0 & 0xffffffffu);
  const unsigned d0 = unsigned(k0 >> 32), d1 = unsigned(k1 >> 32);
  // DMatch::distance is a float; the ratio is a float division stored in a double
  const float f0 = float(d0), f1 = float(d1);
  const double ratio = double(f0 / f1);
  const size_t a = qidx ? size_t(qidx[i]) : size_t(i), b = tidx ? size_t(tidx[j]) : size_t(j);
  const double dx = p0[2 * a] - p1[2 * b], dy = p0[2 * a + 1] - p1[2 * b + 1];
  const double d = dx * dx + dy * dy;
  if (d > minSq && d < maxSq && ratio < ratio_test) {
    atomicMin(&key[j], (static_cast<unsigned long long>(d0) << 32) | unsigned(i));
    atomicMin(&first[j], i);
  }
}

__global__ void k_accept(const unsigned long long* __restrict__ part, int n0, const int* __restrict__ n0_dev, int nslice,
                         const double* __restrict__ p0, const int* __restrict__ qidx, const double* __restrict__ p1,
                         const int* __restrict__ tidx, double ratio_test, double minSq, double maxSq,
                         unsigned long long* __restrict__ key, int* __restrict__ first) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (n0_dev ? *n0_dev : n0)) return;
  accept_query(part, n0, nslice, i, p0, qidx, p1, tidx, ratio_test, minSq, maxSq, key, first);
}

// item blockIdx.y of a batch: its queries, its own key / first block
__global__ void k_accept_items(const sfm::PairItem* __restrict__ items, const int* __restrict__ idx, int nslice,
                               const unsigned long long* __restrict__ part, const double* __restrict__ p1,
                               const int* __restrict__ tidx, double ratio_test, double minSq, double maxSq,
                               unsigned long long* __restrict__ key, int* __restrict__ first) {
  const sfm::PairItem& it = items[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= it.n0) return;
  accept_query(part + it.part_off, it.n0, nslice, i, it.pts, idx + it.idx_off, p1, tidx, ratio_test, minSq, maxSq,
               key + it.key_off, first + it.key_off);
}

__global__ void k_reset_items(const sfm::PairItem* __restrict__ items, int n1, unsigned long long* __restrict__ key,
                              int* __restrict__ first, int* __restrict__ slot) {
  const sfm::PairItem& it = items[blockIdx.y];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n1) { key[it.key_off + t] = kNoKey; first[it.key_off + t] = 0x7fffffff; }
  if (t < it.n0) slot[it.idx_off + t] = 0;
}

__global__ void k_mark_first_items(const sfm::PairItem* __restrict__ items, int n1, const int* __restrict__ first,
                                   int* __restrict__ slot) {
  const sfm::PairItem& it = items[blockIdx.y];
  sfm::mark_first(n1, first + it.key_off, slot + it.idx_off, blockIdx.x * blockDim.x + threadIdx.x);
}

// one workgroup per item
__global__ __launch_bounds__(1024) void k_compact_slots_items(const sfm::PairItem* __restrict__ items,
                                                              const int* __restrict__ slot,
                                                              const unsigned long long* __restrict__ key,
                                                              int* __restrict__ out) {
  const sfm::PairItem& it = items[blockIdx.x];
  int* o = out + it.out_off;
  sfm::compact_slots<false>(it.n0, slot + it.idx_off, key + it.key_off, o, o + it.n0, o + 2 * it.n0);
}

__global__ void k_reset(int n1, unsigned long long* __restrict__ key, int* __restrict__ first, int n0,
                        int* __restrict__ slot) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n1) { key[t] = kNoKey; first[t] = 0x7fffffff; }
  if (t < n0) slot[t] = 0;
}

// Pads descriptors to whole 64-bit words (W a power of two).
int words_for(int nbytes) {
  int W = (nbytes + 7) / 8;
  int p = 1;
  while (p < W) p <<= 1;
  return p;
}

void pack_words(const uint8_t* d, int n, int nbytes, int W, uint64_t* out) {
  if (nbytes == 8 * W) {
    std::memcpy(out, d, size_t(n) * nbytes);
    return;
  }
  std::memset(out, 0, size_t(n) * W * 8);
  for (int i = 0; i < n; ++i) std::memcpy(out + size_t(i) * W, d + size_t(i) * nbytes, nbytes);
}

// CMap::getRepresentativeDescriptors (CMap.cpp:345-381): one wavefront per
// map point; lane r owns rows r, r+64, ... of the point's descriptor matrix
// and sums its Hamming distances to every row (the reference's column sums
// of the symmetric distance matrix: integers, exact in its float), then a
// wave argmin keeps the lowest row on ties (the reference's strict `<` scan).
// Row k's words are wave-uniform loads (one line per instruction).
template <int W>
__global__ __launch_bounds__(64) void k_repr(const uint64_t* __restrict__ d, const int* __restrict__ off, int n_pts,
                                             int* __restrict__ best) {
  const int p = blockIdx.x, l = threadIdx.x;
  if (p >= n_pts) return;
  const int r0 = off[p], k = off[p + 1] - r0;
  const uint64_t* dp = d + size_t(r0) * W;
  const int b = sfm::repr_row<W>(k, l, [dp](int r) { return dp + size_t(r) * W; });
  if (l == 0) best[p] = b;
}

}  // namespace

// ---------------------------------------------------------------------------
// the handle

struct MatchFrame {
  int n = 0;
  DevArr<uint64_t> desc;      // [n][W]; one allocation with the two below
  double* pts = nullptr;      // [n][2] undistorted (CFrame::getPointsAt), right after desc
  double* ptsd = nullptr;     // [n][2] distorted (CFrame::getPointsDistorted), right after pts
};

// The stream first: members are destroyed in reverse order, so it goes last.
struct sfm_matcher {
  Stream stream;
  std::vector<MatchFrame> kf;  // keyframe store (sfm_matcher_store_keyframe)
  int device = 0;
  int desc_bytes = 64, W = 8;
  int n_cu = 256;
  Event ev[3];
  Event ev_rows;              // matcher_keyframe_rows: the keyframe store's uploads are done
  MatchFrame frame[2];        // [prev, curr] after the swap
  int cur = 1;                // index of the current frame in frame[]
  int frames_pushed = 0;
  // pooled scratch (grow-only)
  std::map<std::string, DevBuf> dev;
  std::map<std::string, PinBuf> pin;
  float last_knn_ms = 0.f, last_total_ms = 0.f;
};

namespace {

template <typename T>
T* dbuf(sfm_matcher* h, const char* name, size_t count, int* rc) {
  const size_t bytes = std::max<size_t>(1, count) * sizeof(T);
  DevBuf& b = h->dev[name];
  if (b.reserve(bytes, std::max(bytes, size_t(4096)) * 3 / 2, h->stream))
    *rc = fail(SFM_ENOMEM, "hipMalloc failed (matcher scratch)");
  return b.as<T>();
}

template <typename T>
T* pbuf(sfm_matcher* h, const char* name, size_t count, int* rc) {
  const size_t bytes = std::max<size_t>(1, count) * sizeof(T);
  PinBuf& b = h->pin[name];
  if (b.reserve(bytes, std::max(bytes, size_t(4096)) * 3 / 2, h->stream))
    *rc = fail(SFM_ENOMEM, "hipHostMalloc failed (matcher staging)");
  return b.as<T>();
}

// Room for `need` rows of `row_bytes` in a frame's one allocation, `want`
// rows when it has to grow (the rows it held are dropped).
int frame_reserve(sfm_matcher* h, MatchFrame& f, int need, size_t want, size_t row_bytes, const char* what) {
  const size_t bytes = size_t(std::max(need, 1)) * row_bytes;
  if (f.desc.bytes() < bytes) f.pts = f.ptsd = nullptr;
  if (f.desc.reserve(bytes, want * row_bytes, h->stream))
    return fail(SFM_ENOMEM, std::string("hipMalloc failed (") + what + ")");
  return 0;
}

// Train slices: enough workgroups to put ~8 waves on every CU, each slice
// at least 64 rows (one row per lane-step of every wave is not worth less).
// qb: the call's query blocks (of kQ rows), all items of a batch together.
int slices_for_blocks(const sfm_matcher* h, long long qb, int n1) {
  const long long want = std::max<long long>(1, (2 * h->n_cu + qb - 1) / qb);
  const int most = std::max(1, n1 / 64);
  return int(std::min<long long>(want, most));
}

int slices_for(const sfm_matcher* h, int n0, int n1) { return slices_for_blocks(h, (n0 + kQ - 1) / kQ, n1); }

int launch_knn(sfm_matcher* h, const uint64_t* q, const int* qidx, int n0, const uint64_t* tr, const int* tidx,
               int n1, unsigned long long* part, int nslice) {
  const int slice = (n1 + nslice - 1) / nslice;
  dim3 grid((n0 + kQ - 1) / kQ, nslice);
  switch (h->W) {
#define CASE(w)                                                                                       \
  case w:                                                                                             \
    if (tidx) k_knn2_part<w, true><<<grid, kQ * kWaves, 0, h->stream>>>(q, qidx, n0, tr, tidx, n1, slice, part); \
    else k_knn2_part<w, false><<<grid, kQ * kWaves, 0, h->stream>>>(q, qidx, n0, tr, tidx, n1, slice, part);     \
    break;
    CASE(1) CASE(2) CASE(4) CASE(8) CASE(16) CASE(32) CASE(64)
#undef CASE
    default: return fail(SFM_EINVAL, "descriptor width must be <= 512 bytes");
  }
  return 0;
}

// One match: queries (q, qidx, p0) against trains (tr, tidx, p1) already on
// the device; results (query, train) in subset-local indices into the pinned
// buffer `res` ([2 * n0 + 1]: idx0 | idx1 | count) after the stream sync.
// The kernels alone (no download, no synchronisation): the (query, train)
// pairs and their count land in the device buffer *out_dev ([2 n0 + 1]).
int run_match_async(sfm_matcher* h, const uint64_t* q, const int* qidx, const double* p0, int n0, const uint64_t* tr,
                    const int* tidx, const double* p1, int n1, double ratio, double mn, double mx, int** out_dev,
                    const int* n0_dev = nullptr) {
  int rc = 0;
  const int nslice = slices_for(h, n0, n1);
  auto* part = dbuf<unsigned long long>(h, "part", 2 * size_t(n0) * nslice, &rc);
  auto* key = dbuf<unsigned long long>(h, "key", size_t(n1), &rc);
  int* first = dbuf<int>(h, "first", size_t(n1), &rc);
  int* slot = dbuf<int>(h, "slot", size_t(n0), &rc);
  int* out = dbuf<int>(h, "out", 2 * size_t(n0) + 1, &rc);
  if (rc) return rc;
  hipStream_t s = h->stream;
  hipEventRecord(h->ev[0], s);
  k_reset<<<(std::max(n0, n1) + 255) / 256, 256, 0, s>>>(n1, key, first, n0, slot);
  if ((rc = launch_knn(h, q, qidx, n0, tr, tidx, n1, part, nslice))) return rc;
  hipEventRecord(h->ev[1], s);
  k_accept<<<(n0 + 255) / 256, 256, 0, s>>>(part, n0, n0_dev, nslice, p0, qidx, p1, tidx, ratio, mn * mn, mx * mx, key,
                                             first);
  sfm::k_mark_first<<<(n1 + 255) / 256, 256, 0, s>>>(n1, first, slot);
  sfm::k_compact_slots<false><<<1, 1024, 0, s>>>(n0, slot, key, out, out + n0, out + 2 * n0);
  hipEventRecord(h->ev[2], s);
  *out_dev = out;
  return 0;
}

int run_match(sfm_matcher* h, const uint64_t* q, const int* qidx, const double* p0, int n0, const uint64_t* tr,
              const int* tidx, const double* p1, int n1, double ratio, double mn, double mx, int** res_out,
              const int* n0_dev = nullptr) {
  int rc = 0;
  int* res = pbuf<int>(h, "res", 2 * size_t(n0) + 1, &rc);
  if (rc) return rc;
  int* out = nullptr;
  if ((rc = run_match_async(h, q, qidx, p0, n0, tr, tidx, p1, n1, ratio, mn, mx, &out, n0_dev))) return rc;
  hipStream_t s = h->stream;
  hipMemcpyAsync(res, out, (2 * size_t(n0) + 1) * sizeof(int), hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess) return fail(SFM_EIO, "matcher kernels failed");
  hipEventElapsedTime(&h->last_knn_ms, h->ev[0], h->ev[1]);
  hipEventElapsedTime(&h->last_total_ms, h->ev[0], h->ev[2]);
  *res_out = res;
  return 0;
}

// sfm_track_pnp: the matches (query k -> prev keypoint pidx[out[k]], its map
// point pt3d[.]; train -> current keypoint out[n0 + k]) into PnP's object
// (the map point) and image (the current keypoint) arrays, with the match's
// map point and keypoint kept for the inlier lists; thread 0 copies the count
// into the result block's head.
__global__ void k_track_gather(const int* __restrict__ out, int n0, const int* __restrict__ pidx,
                               const int* __restrict__ pt3d, const double* __restrict__ X,
                               const double* __restrict__ pts, double* __restrict__ obj, double* __restrict__ img,
                               int* __restrict__ m3, int* __restrict__ kp, int* __restrict__ head) {
  const int m = out[2 * n0];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) head[0] = m;
  if (k >= m) return;
  const int p = pt3d[pidx[out[k]]], c = out[n0 + k];
  obj[3 * k] = X[3 * size_t(p)];
  obj[3 * k + 1] = X[3 * size_t(p) + 1];
  obj[3 * k + 2] = X[3 * size_t(p) + 2];
  img[2 * k] = pts[2 * c];
  img[2 * k + 1] = pts[2 * c + 1];
  m3[k] = p;
  kp[k] = c;
}

bool ok_ratio_window(double ratio, double mn, double mx) {
  return std::isfinite(ratio) && std::isfinite(mn) && std::isfinite(mx);
}

// every idx[i], i < n, is a row of a frame of `rows` rows
bool rows_in_range(const int32_t* idx, int32_t n, int rows) {
  for (int32_t i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= rows) return false;
  return true;
}

// run_match's result block ([2 n0 + 1]: query | train | count) into the caller's arrays
void copy_matches(const int* res, int n0, int32_t* idx0, int32_t* idx1, int32_t* n_matches) {
  const int m = res[2 * n0];
  std::memcpy(idx0, res, sizeof(int) * size_t(m));
  std::memcpy(idx1, res + n0, sizeof(int) * size_t(m));
  *n_matches = m;
}

// CSfM::mapping's point creation (CSfM.cpp:138-176) for B older keyframes
// against one set of the new keyframe's rows, up to the first pair that keeps
// a point; sfm_matcher_pair_points is B = 1.  Per pair b: the member-window
// match of rows idx0[idx0_off[b] .. idx0_off[b + 1]) of keyframe slot0[b]
// with rows idx1 of f1, the triangulation and the filter through pa[b]
// (mappoint_kernels.hip), all on the resident rows.  One staged upload (item
// table | per-pair matrices | index lists), eight launches whatever B, one
// download (first | kept [B] | matched [B] | the first productive pair's
// matches), one synchronisation.  The caller has checked slots and index
// lists, composed pa, found a row in idx0 and two in idx1 and set the device.
int pair_points_run(sfm_matcher* h, int B_, const int32_t* slot0, const int32_t* idx0, const int32_t* idx0_off,
                    const MatchFrame& f1, const int32_t* idx1, int n1, double ratio_test, double min_distance,
                    double max_distance, const sfm::PairArgs* pa, int capacity, int32_t* first, int32_t* m0,
                    int32_t* m1, double* X, int32_t* n_kept, int32_t* n_matched) {
  int rc = 0;
  const size_t B = size_t(B_);
  const int total = idx0_off[B];
  int max_n0 = 0;
  long long qb_total = 0;
  for (size_t b = 0; b < B; ++b) {
    const int n0 = idx0_off[b + 1] - idx0_off[b];
    max_n0 = std::max(max_n0, n0);
    qb_total += (n0 + kQ - 1) / kQ;
  }
  const int nslice = slices_for_blocks(h, qb_total, n1);
  const int slice = (n1 + nslice - 1) / nslice;
  // stage (8-B units): item table | matrices | idx0 (all items) | idx1
  static_assert(sizeof(sfm::PairItem) % 8 == 0 && sizeof(sfm::PairArgs) % 8 == 0, "staged in 8-B units");
  const size_t w_items = B * sizeof(sfm::PairItem) / 8, w_pa = B * sizeof(sfm::PairArgs) / 8;
  const size_t w_idx = (size_t(total) + size_t(n1) + 1) / 2;
  const size_t w_stage = w_items + w_pa + w_idx;
  // result block: head (first | kept [B] | matched [B], even) | m0 [cap] | m1 [cap] | X [cap][3]
  const size_t cap = size_t(std::min(max_n0, n1));
  const size_t hi = (2 * B + 2) & ~size_t(1);
  const size_t blk = hi / 2 + cap + 3 * cap;  // in doubles
  auto* st = pbuf<uint64_t>(h, "pfstage", w_stage, &rc);
  auto* dst = dbuf<uint64_t>(h, "dpfstage", w_stage, &rc);
  auto* part = dbuf<unsigned long long>(h, "part", 2 * size_t(total) * nslice, &rc);
  auto* key = dbuf<unsigned long long>(h, "key", B * size_t(n1), &rc);
  int* dfirst = dbuf<int>(h, "first", B * size_t(n1), &rc);
  int* slot = dbuf<int>(h, "slot", size_t(total), &rc);
  int* out = dbuf<int>(h, "out", 2 * size_t(total) + B, &rc);
  double* dXall = dbuf<double>(h, "ppX", 3 * size_t(total), &rc);
  int* dks = dbuf<int>(h, "ppks", 2 * size_t(total), &rc);
  double* dblk = dbuf<double>(h, "pfblk", blk, &rc);
  double* hblk = pbuf<double>(h, "pfblkh", blk, &rc);
  if (rc) return rc;
  hipStream_t s = h->stream;
  hipStreamSynchronize(s);  // (the pinned stage may feed an earlier copy)
  auto* items = reinterpret_cast<sfm::PairItem*>(st);
  for (size_t b = 0; b < B; ++b) {
    const MatchFrame& f0 = h->kf[size_t(slot0[b])];
    sfm::PairItem& it = items[b];
    it.desc = f0.desc;
    it.pts = f0.pts;
    it.n0 = idx0_off[b + 1] - idx0_off[b];
    it.idx_off = idx0_off[b];
    it.out_off = 2 * idx0_off[b] + int(b);
    it.pad = 0;
    it.part_off = 2ll * idx0_off[b] * nslice;
    it.key_off = (long long)(b) * n1;
    it.x_off = 3ll * idx0_off[b];
  }
  std::memcpy(st + w_items, pa, B * sizeof(sfm::PairArgs));
  int* ix = reinterpret_cast<int*>(st + w_items + w_pa);
  std::memcpy(ix, idx0, sizeof(int) * size_t(total));
  std::memcpy(ix + total, idx1, sizeof(int) * size_t(n1));
  hipMemcpyAsync(dst, st, w_stage * 8, hipMemcpyHostToDevice, s);
  const auto* ditems = reinterpret_cast<const sfm::PairItem*>(dst);
  const auto* dpa = reinterpret_cast<const sfm::PairArgs*>(dst + w_items);
  const int* dix = reinterpret_cast<const int*>(dst + w_items + w_pa);
  const int* dtix = dix + total;
  const unsigned by = unsigned(B_);
  hipEventRecord(h->ev[0], s);
  k_reset_items<<<dim3((std::max(max_n0, n1) + 255) / 256, by), 256, 0, s>>>(ditems, n1, key, dfirst, slot);
  const dim3 grid((max_n0 + kQ - 1) / kQ, nslice, by);
  switch (h->W) {
#define CASE(w) \
  case w: k_knn2_part_items<w><<<grid, kQ * kWaves, 0, s>>>(ditems, dix, f1.desc, dtix, n1, slice, part); break;
    CASE(1) CASE(2) CASE(4) CASE(8) CASE(16) CASE(32) CASE(64)
#undef CASE
    default: return fail(SFM_EINVAL, "descriptor width must be <= 512 bytes");
  }
  hipEventRecord(h->ev[1], s);
  k_accept_items<<<dim3((max_n0 + 255) / 256, by), 256, 0, s>>>(ditems, dix, nslice, part, f1.pts, dtix, ratio_test,
                                                                 min_distance * min_distance,
                                                                 max_distance * max_distance, key, dfirst);
  k_mark_first_items<<<dim3((n1 + 255) / 256, by), 256, 0, s>>>(ditems, n1, dfirst, slot);
  k_compact_slots_items<<<by, 1024, 0, s>>>(ditems, slot, key, out);
  int* dhead = reinterpret_cast<int*>(dblk);
  sfm::launch_pair_points_first(s, ditems, dpa, B_, max_n0, out, dix, dtix, f1.pts, dXall, dks, dks + total, dhead,
                                dhead + hi, dhead + hi + cap, dblk + hi / 2 + cap);
  hipEventRecord(h->ev[2], s);
  hipMemcpyAsync(hblk, dblk, sizeof(double) * blk, hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess) return fail(SFM_EIO, "point-creation kernels failed");
  hipEventElapsedTime(&h->last_knn_ms, h->ev[0], h->ev[1]);
  hipEventElapsedTime(&h->last_total_ms, h->ev[0], h->ev[2]);
  const int* hh = reinterpret_cast<const int*>(hblk);
  *first = hh[0];
  std::memcpy(n_kept, hh + 1, sizeof(int) * B);
  std::memcpy(n_matched, hh + 1 + B, sizeof(int) * B);
  if (hh[0] < 0) return 0;
  const int kept = n_kept[hh[0]];
  if (kept > capacity)
    return fail(SFM_EINVAL, "capacity " + std::to_string(capacity) + " < " + std::to_string(kept) + " kept matches");
  std::memcpy(m0, hh + hi, sizeof(int) * size_t(kept));
  std::memcpy(m1, hh + hi + cap, sizeof(int) * size_t(kept));
  std::memcpy(X, hblk + hi / 2 + cap, sizeof(double) * 3 * size_t(kept));
  return 0;
}

}  // namespace

namespace sfm {
// pnp_kernels.hip / map_store.hip (sfm_track_pnp)
int pnp_ransac_dev(hipStream_t s, const int* d_n, int gate, const double* d_obj, const double* d_img, const double* K9,
                   int iterations, double reproj_err, double confidence, int* d_sub, double* d_model, int* d_cnt,
                   int* d_res, int* d_inl);
int pnp_max_iters();
int pnp_model_size();
const double* map_points_dev(sfm_map* h, int32_t* n_pts, int* device);
// For sfm_map_match_frame (map_store.hip): queries already on the device
// (descriptor words q, positions p0; produced on another stream, ordered
// after the event `after`) against a subset of the CURRENT frame's keypoints
// (d_train_idx, frame-local, on the device, checked by the caller against
// matcher_current_n); the (query, train) pairs in subset-local indices, as
// sfm_matcher_match returns them, in *res (pinned, valid after this call).
// No upload and no synchronisation before the kernels.
int matcher_match_current_dev(sfm_matcher* h, hipEvent_t after, const uint64_t* q, const double* p0, int n0,
                              const int32_t* d_n0, const int32_t* d_train_idx, int n1, double ratio, double mn,
                              double mx, int** res) {
  if (h->frames_pushed < 1) return fail(SFM_EINVAL, "push the current frame first");
  if (!ok_ratio_window(ratio, mn, mx)) return fail(SFM_EINVAL, "non-finite threshold");
  const MatchFrame& fc = h->frame[h->cur];
  if (after && hipStreamWaitEvent(h->stream, after, 0) != hipSuccess) return fail(SFM_EIO, "stream wait failed");
  return run_match(h, q, nullptr, p0, n0, fc.desc, d_train_idx, fc.pts, n1, ratio, mn, mx, res, d_n0);
}
int matcher_current_n(const sfm_matcher* h) { return h->frames_pushed < 1 ? -1 : h->frame[h->cur].n; }
int matcher_words(const sfm_matcher* h) { return h->W; }
int matcher_device(const sfm_matcher* h) { return h->device; }
int matcher_desc_bytes(const sfm_matcher* h) { return h->desc_bytes; }

// For sfm_map_add_keyframe_rows (map_store.hip): the descriptor words of
// keyframe `slot` ([*n][matcher_words]) and an event after which they are
// complete (the store's upload runs on the matcher's stream).
int matcher_keyframe_rows(sfm_matcher* h, int32_t slot, const uint64_t** desc, int* n, hipEvent_t* ready) {
  if (slot < 0 || size_t(slot) >= h->kf.size()) return fail(SFM_EINVAL, "keyframe slot not stored");
  if (h->ev_rows.create(hipEventDisableTiming) != hipSuccess) return fail(SFM_EIO, "hipEventCreate failed");
  if (hipEventRecord(h->ev_rows, h->stream) != hipSuccess) return fail(SFM_EIO, "hipEventRecord failed");
  *desc = h->kf[size_t(slot)].desc;
  *n = h->kf[size_t(slot)].n;
  *ready = h->ev_rows;
  return 0;
}

// For sfm_frame_detect (frame_kernels.hip): sfm_matcher_push_frame in two
// halves around a device-side fill.  begin sizes the slot push_frame would
// overwrite (the previous frame's: call it only once the new frame is known
// to be accepted) for m keypoints, laid out as push_frame does; commit is
// the prev/curr swap.
int matcher_install_begin(sfm_matcher* h, int n, int m, MatchSlot* out) {
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  MatchFrame& f = h->frame[h->cur ^ 1];
  int rc = frame_reserve(h, f, m, size_t(std::max(m, 1024)) * 3 / 2, h->W * 8 + 32, "matcher frame");
  if (rc) return rc;
  out->scratch = dbuf<int>(h, "install", size_t(n) + 1, &rc);
  if (rc) return rc;
  out->desc = f.desc;
  out->pts = reinterpret_cast<double*>(f.desc + size_t(m) * h->W);
  out->ptsd = out->pts + 2 * size_t(m);
  out->stream = h->stream;
  return 0;
}
void matcher_install_commit(sfm_matcher* h, int m) {
  h->cur ^= 1;
  MatchFrame& f = h->frame[h->cur];
  f.n = m;
  f.pts = reinterpret_cast<double*>(f.desc + size_t(m) * h->W);
  f.ptsd = f.pts + 2 * size_t(m);
  ++h->frames_pushed;
}
}  // namespace sfm

extern "C" {

int sfm_matcher_create(int32_t device, int32_t desc_bytes, sfm_matcher** out) {
  if (!out) return fail(SFM_EINVAL, "out is NULL");
  *out = nullptr;
  if (desc_bytes <= 0 || desc_bytes > 512) return fail(SFM_EINVAL, "desc_bytes must be in 1..512");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(SFM_ENODEV, "no HIP device visible");
  if (device < 0 || device >= n) return fail(SFM_EINVAL, "device ordinal out of range");
  if (hipSetDevice(device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  auto* h = new sfm_matcher();
  h->device = device;
  h->desc_bytes = desc_bytes;
  h->W = words_for(desc_bytes);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    h->n_cu = prop.multiProcessorCount;
  if (h->stream.create(hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return fail(SFM_EIO, "hipStreamCreate failed");
  }
  for (auto& e : h->ev) (void)e.create(hipEventDefault);
  *out = h;
  return 0;
}

int sfm_matcher_destroy(sfm_matcher* h) {
  if (!h) return 0;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  delete h;
  return 0;
}

int sfm_matcher_push_frame(sfm_matcher* h, const double* pts, const double* pts_distorted, const uint8_t* desc,
                           int32_t n) {
  SFM_TRACE("sfm_matcher_push_frame");
  if (!h) return fail(SFM_EINVAL, "handle is NULL");
  if (n < 0 || (n > 0 && (!pts || !desc))) return fail(SFM_EINVAL, "bad frame arguments");
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  // the current frame becomes the previous one (CSfM.cpp:626-629)
  h->cur ^= 1;
  MatchFrame& f = h->frame[h->cur];
  int rc = frame_reserve(h, f, n, size_t(std::max(n, 1024)) * 3 / 2, h->W * 8 + 32, "matcher frame");
  if (rc) return rc;
  f.n = n;
  // [desc n W | pts 2n | ptsd 2n] as laid out in the stage: one copy
  f.pts = reinterpret_cast<double*>(f.desc + size_t(n) * h->W);
  f.ptsd = f.pts + 2 * size_t(n);
  if (n) {
    // staging: one pinned block per frame slot (the previous upload from it
    // may still be in flight only for the other slot)
    const char* nm = h->cur ? "stage1" : "stage0";
    const size_t words = size_t(n) * h->W;
    auto* st = pbuf<uint64_t>(h, nm, words + 4 * size_t(n), &rc);
    if (rc) return rc;
    hipStreamSynchronize(h->stream);   // the stage may feed an earlier copy
    pack_words(desc, n, h->desc_bytes, h->W, st);
    double* sp = reinterpret_cast<double*>(st + words);
    std::memcpy(sp, pts, 16 * size_t(n));
    std::memcpy(sp + 2 * size_t(n), pts_distorted ? pts_distorted : pts, 16 * size_t(n));
    hipMemcpyAsync(f.desc, st, words * 8 + 32 * size_t(n), hipMemcpyHostToDevice, h->stream);
  }
  ++h->frames_pushed;
  return 0;
}

int sfm_matcher_match_subset(sfm_matcher* h, const int32_t* prev_idx, int32_t n_prev, const int32_t* curr_idx,
                             int32_t n_curr, double ratio_test, double min_distance, double max_distance,
                             int32_t* prev_match, int32_t* curr_match, int32_t* n_matches) {
  SFM_TRACE("sfm_matcher_match_subset");
  if (!h || !n_matches) return fail(SFM_EINVAL, "NULL argument");
  *n_matches = 0;
  if (h->frames_pushed < 2) return fail(SFM_EINVAL, "push the previous and the current frame first");
  if (n_prev < 0 || n_curr < 0 || (n_prev && !prev_idx) || (n_curr && !curr_idx))
    return fail(SFM_EINVAL, "bad index lists");
  if (!ok_ratio_window(ratio_test, min_distance, max_distance)) return fail(SFM_EINVAL, "non-finite threshold");
  const MatchFrame& fp = h->frame[h->cur ^ 1];
  const MatchFrame& fc = h->frame[h->cur];
  if (!rows_in_range(prev_idx, n_prev, fp.n)) return fail(SFM_EINVAL, "prev index out of range");
  if (!rows_in_range(curr_idx, n_curr, fc.n)) return fail(SFM_EINVAL, "curr index out of range");
  if (n_prev == 0 || n_curr < 2) return 0;  // reference UB with < 2 train rows: no matches
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  int rc = 0;
  int* ix = pbuf<int>(h, "idx", size_t(n_prev) + n_curr, &rc);
  int* dix = dbuf<int>(h, "didx", size_t(n_prev) + n_curr, &rc);
  if (rc) return rc;
  hipStreamSynchronize(h->stream);
  std::memcpy(ix, prev_idx, sizeof(int) * size_t(n_prev));
  std::memcpy(ix + n_prev, curr_idx, sizeof(int) * size_t(n_curr));
  hipMemcpyAsync(dix, ix, sizeof(int) * (size_t(n_prev) + n_curr), hipMemcpyHostToDevice, h->stream);
  int* res = nullptr;
  // undistorted positions (CFrame::getPointsAt, CTracker.cpp:375-376)
  if ((rc = run_match(h, fp.desc, dix, fp.pts, n_prev, fc.desc, dix + n_prev, fc.pts, n_curr, ratio_test,
                      min_distance, max_distance, &res)))
    return rc;
  copy_matches(res, n_prev, prev_match, curr_match, n_matches);
  // frame-global indices (CTracker.cpp:406-407, 412)
  for (int k = 0; k < *n_matches; ++k) {
    prev_match[k] = prev_idx[prev_match[k]];
    curr_match[k] = curr_idx[curr_match[k]];
  }
  return 0;
}

int sfm_matcher_match_frames(sfm_matcher* h, int32_t distorted, double ratio_test, double min_distance,
                             double max_distance, int32_t* prev_idx, int32_t* curr_idx, int32_t* n_matches) {
  if (!h || !n_matches) return fail(SFM_EINVAL, "NULL argument");
  *n_matches = 0;
  if (h->frames_pushed < 2) return fail(SFM_EINVAL, "push the previous and the current frame first");
  if (!ok_ratio_window(ratio_test, min_distance, max_distance)) return fail(SFM_EINVAL, "non-finite threshold");
  const MatchFrame& fp = h->frame[h->cur ^ 1];
  const MatchFrame& fc = h->frame[h->cur];
  if (fp.n == 0 || fc.n < 2) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  int* res = nullptr;
  int rc = run_match(h, fp.desc, nullptr, distorted ? fp.ptsd : fp.pts, fp.n, fc.desc, nullptr,
                     distorted ? fc.ptsd : fc.pts, fc.n, ratio_test, min_distance, max_distance, &res);
  if (rc) return rc;
  copy_matches(res, fp.n, prev_idx, curr_idx, n_matches);
  return 0;
}

int sfm_matcher_match(sfm_matcher* h, const double* pts0, const uint8_t* desc0, int32_t n0, const double* pts1,
                      const uint8_t* desc1, int32_t n1, double ratio_test, double min_distance, double max_distance,
                      int32_t* idx0, int32_t* idx1, int32_t* n_matches) {
  SFM_TRACE("sfm_matcher_match");
  if (!h || !n_matches) return fail(SFM_EINVAL, "NULL argument");
  *n_matches = 0;
  if (n0 < 0 || n1 < 0) return fail(SFM_EINVAL, "negative size");
  if ((n0 && (!pts0 || !desc0)) || (n1 && (!pts1 || !desc1))) return fail(SFM_EINVAL, "NULL array");
  if (!ok_ratio_window(ratio_test, min_distance, max_distance)) return fail(SFM_EINVAL, "non-finite threshold");
  if (n0 == 0 || n1 < 2) return 0;  // reference UB with < 2 train rows: no matches
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  int rc = 0;
  const size_t w0 = size_t(n0) * h->W, w1 = size_t(n1) * h->W;
  auto* st = pbuf<uint64_t>(h, "in", w0 + w1 + 2 * (size_t(n0) + n1), &rc);
  auto* d = dbuf<uint64_t>(h, "din", w0 + w1 + 2 * (size_t(n0) + n1), &rc);
  if (rc) return rc;
  hipStreamSynchronize(h->stream);
  pack_words(desc0, n0, h->desc_bytes, h->W, st);
  pack_words(desc1, n1, h->desc_bytes, h->W, st + w0);
  double* sp = reinterpret_cast<double*>(st + w0 + w1);
  std::memcpy(sp, pts0, 16 * size_t(n0));
  std::memcpy(sp + 2 * size_t(n0), pts1, 16 * size_t(n1));
  hipMemcpyAsync(d, st, (w0 + w1 + 2 * (size_t(n0) + n1)) * 8, hipMemcpyHostToDevice, h->stream);
  const double* dp = reinterpret_cast<const double*>(d + w0 + w1);
  int* res = nullptr;
  if ((rc = run_match(h, d, nullptr, dp, n0, d + w0, nullptr, dp + 2 * size_t(n0), n1, ratio_test, min_distance,
                      max_distance, &res)))
    return rc;
  copy_matches(res, n0, idx0, idx1, n_matches);
  return 0;
}

// Keyframe store (CSfM::mapping's keyframe-pair matching, CSfM.cpp:141-221):
// slot `slot` takes pts [n][2] and desc [n][desc_bytes] once, resident.
int sfm_matcher_store_keyframe(sfm_matcher* h, int32_t slot, const double* pts, const uint8_t* desc, int32_t n) {
  SFM_TRACE("sfm_matcher_store_keyframe");
  if (!h) return fail(SFM_EINVAL, "handle is NULL");
  if (slot < 0 || slot > (1 << 20) || n < 0 || (n > 0 && (!pts || !desc))) return fail(SFM_EINVAL, "bad keyframe arguments");
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  if (size_t(slot) >= h->kf.size()) h->kf.resize(size_t(slot) + 1);
  MatchFrame& f = h->kf[size_t(slot)];
  int rc = frame_reserve(h, f, n, size_t(std::max(n, 1)), h->W * 8 + 16, "matcher keyframe");
  if (rc) return rc;
  f.n = n;
  f.pts = reinterpret_cast<double*>(f.desc + size_t(n) * h->W);
  f.ptsd = f.pts;
  if (n) {
    const size_t words = size_t(n) * h->W;
    auto* st = pbuf<uint64_t>(h, "kfstage", words + 2 * size_t(n), &rc);
    if (rc) return rc;
    hipStreamSynchronize(h->stream);
    pack_words(desc, n, h->desc_bytes, h->W, st);
    std::memcpy(st + words, pts, 16 * size_t(n));
    hipMemcpyAsync(f.desc, st, words * 8 + 16 * size_t(n), hipMemcpyHostToDevice, h->stream);
  }
  return 0;
}

// sfm_matcher_match on keyframe rows: query rows q_idx of keyframe q_slot
// (positions q_pts [n_q][2] when given -- then q_idx must not repeat --,
// else the keyframe's own), train rows t_idx of keyframe t_slot; indices out
// are subset-local (into q_idx / t_idx), as sfm_matcher_match returns them.
int sfm_matcher_match_keyframes(sfm_matcher* h, int32_t q_slot, const int32_t* q_idx, int32_t n_q, const double* q_pts,
                                int32_t t_slot, const int32_t* t_idx, int32_t n_t, double ratio_test,
                                double min_distance, double max_distance, int32_t* idx0, int32_t* idx1,
                                int32_t* n_matches) {
  SFM_TRACE("sfm_matcher_match_keyframes");
  if (!h || !n_matches || !idx0 || !idx1) return fail(SFM_EINVAL, "NULL argument");
  *n_matches = 0;
  if (q_slot < 0 || t_slot < 0 || size_t(q_slot) >= h->kf.size() || size_t(t_slot) >= h->kf.size())
    return fail(SFM_EINVAL, "keyframe slot not stored");
  if (n_q < 0 || n_t < 0 || (n_q && !q_idx) || (n_t && !t_idx)) return fail(SFM_EINVAL, "bad index lists");
  if (!ok_ratio_window(ratio_test, min_distance, max_distance)) return fail(SFM_EINVAL, "non-finite threshold");
  const MatchFrame& fq = h->kf[size_t(q_slot)];
  const MatchFrame& ft = h->kf[size_t(t_slot)];
  if (!rows_in_range(q_idx, n_q, fq.n)) return fail(SFM_EINVAL, "query index out of range");
  if (q_pts) {
    std::vector<char> seen(size_t(fq.n), 0);
    for (int32_t i = 0; i < n_q; ++i) {
      if (seen[size_t(q_idx[i])]) return fail(SFM_EINVAL, "query index repeated with given positions");
      seen[size_t(q_idx[i])] = 1;
    }
  }
  if (!rows_in_range(t_idx, n_t, ft.n)) return fail(SFM_EINVAL, "train index out of range");
  if (n_q == 0 || n_t < 2) return 0;  // reference UB with < 2 train rows: no matches
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  int rc = 0;
  // stage: q_idx | t_idx | (8-B aligned) query positions at their rows
  const size_t ni = (size_t(n_q) + n_t + 1) & ~size_t(1);
  const size_t np = q_pts ? 2 * size_t(fq.n) : 0;
  auto* st = pbuf<int>(h, "kfidx", ni + 2 * np, &rc);
  auto* d = dbuf<int>(h, "dkfidx", ni + 2 * np, &rc);
  if (rc) return rc;
  hipStreamSynchronize(h->stream);
  std::memcpy(st, q_idx, sizeof(int) * size_t(n_q));
  std::memcpy(st + n_q, t_idx, sizeof(int) * size_t(n_t));
  double* sp = reinterpret_cast<double*>(st + ni);
  if (q_pts)
    for (int32_t i = 0; i < n_q; ++i) {
      sp[2 * size_t(q_idx[i])] = q_pts[2 * size_t(i)];
      sp[2 * size_t(q_idx[i]) + 1] = q_pts[2 * size_t(i) + 1];
    }
  hipMemcpyAsync(d, st, sizeof(int) * (ni + 2 * np), hipMemcpyHostToDevice, h->stream);
  const double* p0 = q_pts ? reinterpret_cast<const double*>(d + ni) : fq.pts;
  int* res = nullptr;
  if ((rc = run_match(h, fq.desc, d, p0, n_q, ft.desc, d + n_q, ft.pts, n_t, ratio_test, min_distance, max_distance,
                      &res)))
    return rc;
  copy_matches(res, n_q, idx0, idx1, n_matches);
  return 0;
}

// CSfM::mapping's point creation for one keyframe pair (CSfM.cpp:138-176):
// pair_points_run with one pair.  (slot0 == slot1 is allowed here.)
int sfm_matcher_pair_points(sfm_matcher* h, int32_t slot0, const int32_t* idx0, int32_t n0, int32_t slot1,
                            const int32_t* idx1, int32_t n1, double ratio_test, double min_distance,
                            double max_distance, const double* K9_0, const double* R9_0, const double* t3_0,
                            const double* K9_1, const double* R9_1, const double* t3_1, double max_err,
                            int32_t capacity, int32_t* m0, int32_t* m1, double* X, int32_t* n_kept,
                            int32_t* n_matched) {
  SFM_TRACE("sfm_matcher_pair_points");
  if (!h || !n_kept || !n_matched || !m0 || !m1 || !X) return fail(SFM_EINVAL, "NULL argument");
  *n_kept = 0;
  *n_matched = 0;
  if (!K9_0 || !R9_0 || !t3_0 || !K9_1 || !R9_1 || !t3_1) return fail(SFM_EINVAL, "NULL matrix");
  if (slot0 < 0 || slot1 < 0 || size_t(slot0) >= h->kf.size() || size_t(slot1) >= h->kf.size())
    return fail(SFM_EINVAL, "keyframe slot not stored");
  if (n0 < 0 || n1 < 0 || capacity < 0 || (n0 && !idx0) || (n1 && !idx1)) return fail(SFM_EINVAL, "bad index lists");
  if (!ok_ratio_window(ratio_test, min_distance, max_distance) || !std::isfinite(max_err))
    return fail(SFM_EINVAL, "non-finite threshold");
  sfm::PairArgs pa;
  if (!sfm::compose_pair(K9_0, R9_0, t3_0, K9_1, R9_1, t3_1, max_err, &pa))
    return fail(SFM_EINVAL, "K must be finite and upper triangular with K[8] = 1, R and t finite");
  const MatchFrame& f1 = h->kf[size_t(slot1)];
  if (!rows_in_range(idx0, n0, h->kf[size_t(slot0)].n))
    return fail(SFM_EINVAL, "row index out of range (older keyframe)");
  if (!rows_in_range(idx1, n1, f1.n)) return fail(SFM_EINVAL, "row index out of range (new keyframe)");
  if (n0 == 0 || n1 < 2) return 0;  // reference UB with < 2 train rows: no matches
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  const int32_t off[2] = {0, n0};
  int32_t first = -1, kept = 0, matched = 0;
  const int rc = pair_points_run(h, 1, &slot0, idx0, off, f1, idx1, n1, ratio_test, min_distance, max_distance, &pa,
                                 capacity, &first, m0, m1, X, &kept, &matched);
  *n_kept = kept;  // (also when the capacity was too small; *n_matched stays 0 then)
  if (rc) return rc;
  *n_matched = matched;
  return 0;
}

// sfm_matcher_pair_points for many older keyframes against one set of the new
// keyframe's rows, up to the first pair that keeps a point: while no pair has
// kept one the caller's unmatched set does not change, so the pairs are
// independent and the first productive one (in the caller's order) is what
// the pair-by-pair loop would have reached.
int sfm_matcher_pair_points_first(sfm_matcher* h, int32_t n_pairs, const int32_t* slot0, const int32_t* idx0,
                                  const int32_t* idx0_off, int32_t slot1, const int32_t* idx1, int32_t n1,
                                  double ratio_test, double min_distance, double max_distance, const double* K9_0,
                                  const double* R9_0, const double* t3_0, const double* K9_1, const double* R9_1,
                                  const double* t3_1, double max_err, int32_t capacity, int32_t* first, int32_t* m0,
                                  int32_t* m1, double* X, int32_t* n_kept, int32_t* n_matched) {
  SFM_TRACE("sfm_matcher_pair_points_first");
  if (!h || !first || !n_kept || !n_matched || !m0 || !m1 || !X) return fail(SFM_EINVAL, "NULL argument");
  *first = -1;
  if (n_pairs < 0 || n_pairs > 65535) return fail(SFM_EINVAL, "n_pairs must be in 0..65535");
  for (int32_t b = 0; b < n_pairs; ++b) n_kept[b] = n_matched[b] = 0;
  if (n_pairs == 0) return 0;
  if (!slot0 || !idx0_off) return fail(SFM_EINVAL, "NULL pair list");
  if (!K9_0 || !R9_0 || !t3_0 || !K9_1 || !R9_1 || !t3_1) return fail(SFM_EINVAL, "NULL matrix");
  if (slot1 < 0 || size_t(slot1) >= h->kf.size()) return fail(SFM_EINVAL, "keyframe slot not stored");
  if (n1 < 0 || capacity < 0 || (n1 && !idx1)) return fail(SFM_EINVAL, "bad index lists");
  if (idx0_off[0] != 0) return fail(SFM_EINVAL, "idx0_off[0] must be 0");
  for (int32_t b = 0; b < n_pairs; ++b)
    if (idx0_off[b + 1] < idx0_off[b]) return fail(SFM_EINVAL, "idx0_off must not decrease");
  const int total = idx0_off[n_pairs];
  if (total && !idx0) return fail(SFM_EINVAL, "bad index lists");
  if (!ok_ratio_window(ratio_test, min_distance, max_distance) || !std::isfinite(max_err))
    return fail(SFM_EINVAL, "non-finite threshold");
  const MatchFrame& f1 = h->kf[size_t(slot1)];
  if (!rows_in_range(idx1, n1, f1.n)) return fail(SFM_EINVAL, "row index out of range (new keyframe)");
  std::vector<sfm::PairArgs> pa;
  pa.resize(size_t(n_pairs));
  for (int32_t b = 0; b < n_pairs; ++b) {
    if (slot0[b] < 0 || size_t(slot0[b]) >= h->kf.size()) return fail(SFM_EINVAL, "keyframe slot not stored");
    if (slot0[b] == slot1) return fail(SFM_EINVAL, "an older keyframe's slot is the new keyframe's");
    if (!rows_in_range(idx0 + idx0_off[b], idx0_off[b + 1] - idx0_off[b], h->kf[size_t(slot0[b])].n))
      return fail(SFM_EINVAL, "row index out of range (older keyframe)");
    if (!sfm::compose_pair(K9_0 + 9 * size_t(b), R9_0 + 9 * size_t(b), t3_0 + 3 * size_t(b), K9_1, R9_1, t3_1, max_err,
                           &pa[size_t(b)]))
      return fail(SFM_EINVAL, "K must be finite and upper triangular with K[8] = 1, R and t finite");
  }
  if (total == 0 || n1 < 2) return 0;  // reference UB with < 2 train rows: no matches
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  return pair_points_run(h, n_pairs, slot0, idx0, idx0_off, f1, idx1, n1, ratio_test, min_distance, max_distance,
                         pa.data(), capacity, first, m0, m1, X, n_kept, n_matched);
}

// The re-finding of new points in one keyframe in between (CSfM.cpp:191-221):
// sfm_matcher_match_keyframes with q_pts = the projections of X, projected on
// the device (k_project_rows) -- one upload, one synchronisation.
int sfm_matcher_refind_points(sfm_matcher* h, int32_t q_slot, const int32_t* q_idx, int32_t n_q, const double* X,
                              const double* K9, const double* R9, const double* t3, int32_t t_slot,
                              const int32_t* t_idx, int32_t n_t, double ratio_test, double min_distance,
                              double max_distance, int32_t* idx0, int32_t* idx1, int32_t* n_matches) {
  SFM_TRACE("sfm_matcher_refind_points");
  if (!h || !n_matches || !idx0 || !idx1) return fail(SFM_EINVAL, "NULL argument");
  *n_matches = 0;
  if (!K9 || !R9 || !t3) return fail(SFM_EINVAL, "NULL matrix");
  if (q_slot < 0 || t_slot < 0 || size_t(q_slot) >= h->kf.size() || size_t(t_slot) >= h->kf.size())
    return fail(SFM_EINVAL, "keyframe slot not stored");
  if (n_q < 0 || n_t < 0 || (n_q && (!q_idx || !X)) || (n_t && !t_idx)) return fail(SFM_EINVAL, "bad index lists");
  if (!ok_ratio_window(ratio_test, min_distance, max_distance)) return fail(SFM_EINVAL, "non-finite threshold");
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(K9[i]) || !std::isfinite(R9[i])) return fail(SFM_EINVAL, "non-finite matrix");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(t3[i])) return fail(SFM_EINVAL, "non-finite matrix");
  const MatchFrame& fq = h->kf[size_t(q_slot)];
  const MatchFrame& ft = h->kf[size_t(t_slot)];
  if (!rows_in_range(q_idx, n_q, fq.n)) return fail(SFM_EINVAL, "query index out of range");
  std::vector<char> seen(size_t(fq.n), 0);
  for (int32_t i = 0; i < n_q; ++i) {
    if (seen[size_t(q_idx[i])]) return fail(SFM_EINVAL, "query index repeated");
    seen[size_t(q_idx[i])] = 1;
  }
  if (!rows_in_range(t_idx, n_t, ft.n)) return fail(SFM_EINVAL, "train index out of range");
  if (n_q == 0 || n_t < 2) return 0;  // reference UB with < 2 train rows: no matches
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  int rc = 0;
  // stage: q_idx | t_idx | (8-B aligned) X
  const size_t ni = (size_t(n_q) + n_t + 1) & ~size_t(1);
  auto* st = pbuf<int>(h, "rfidx", ni + 6 * size_t(n_q), &rc);
  auto* d = dbuf<int>(h, "drfidx", ni + 6 * size_t(n_q), &rc);
  double* duv = dbuf<double>(h, "rfuv", 2 * size_t(fq.n), &rc);
  if (rc) return rc;
  hipStreamSynchronize(h->stream);
  std::memcpy(st, q_idx, sizeof(int) * size_t(n_q));
  std::memcpy(st + n_q, t_idx, sizeof(int) * size_t(n_t));
  std::memcpy(st + ni, X, sizeof(double) * 3 * size_t(n_q));
  hipMemcpyAsync(d, st, sizeof(int) * (ni + 6 * size_t(n_q)), hipMemcpyHostToDevice, h->stream);
  sfm::launch_project_rows(h->stream, n_q, d, reinterpret_cast<const double*>(d + ni), R9, t3, K9, duv);
  int* res = nullptr;
  if ((rc = run_match(h, fq.desc, d, duv, n_q, ft.desc, d + n_q, ft.pts, n_t, ratio_test, min_distance, max_distance,
                      &res)))
    return rc;
  copy_matches(res, n_q, idx0, idx1, n_matches);
  return 0;
}

int sfm_matcher_knn2(sfm_matcher* h, const uint8_t* desc0, int32_t n0, const uint8_t* desc1, int32_t n1,
                     int32_t* best_idx, int32_t* best_dist, int32_t* second_idx, int32_t* second_dist) {
  if (!h) return fail(SFM_EINVAL, "handle is NULL");
  if (n0 < 0 || n1 < 0 || (n0 && !desc0) || (n1 && !desc1)) return fail(SFM_EINVAL, "bad arguments");
  if (n0 == 0) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  int rc = 0;
  const size_t w0 = size_t(n0) * h->W, w1 = size_t(n1) * h->W;
  auto* st = pbuf<uint64_t>(h, "in", w0 + w1, &rc);
  auto* d = dbuf<uint64_t>(h, "din", w0 + w1, &rc);
  const int nslice = n1 > 0 ? slices_for(h, n0, n1) : 1;
  auto* part = dbuf<unsigned long long>(h, "part", 2 * size_t(n0) * nslice, &rc);
  int* out = dbuf<int>(h, "kout", 4 * size_t(n0), &rc);
  int* res = pbuf<int>(h, "kres", 4 * size_t(n0), &rc);
  if (rc) return rc;
  hipStreamSynchronize(h->stream);
  pack_words(desc0, n0, h->desc_bytes, h->W, st);
  if (n1) pack_words(desc1, n1, h->desc_bytes, h->W, st + w0);
  hipMemcpyAsync(d, st, (w0 + w1) * 8, hipMemcpyHostToDevice, h->stream);
  if ((rc = launch_knn(h, d, nullptr, n0, d + w0, nullptr, n1, part, nslice))) return rc;
  k_knn2_merge<<<(n0 + 255) / 256, 256, 0, h->stream>>>(part, n0, nslice, out);
  hipMemcpyAsync(res, out, 4 * size_t(n0) * sizeof(int), hipMemcpyDeviceToHost, h->stream);
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(SFM_EIO, "matcher kernels failed");
  std::memcpy(best_idx, res, n0 * sizeof(int));
  std::memcpy(best_dist, res + n0, n0 * sizeof(int));
  std::memcpy(second_idx, res + 2 * size_t(n0), n0 * sizeof(int));
  std::memcpy(second_dist, res + 3 * size_t(n0), n0 * sizeof(int));
  return 0;
}

int sfm_matcher_last_time(sfm_matcher* h, double* ms2) {
  if (!h || !ms2) return fail(SFM_EINVAL, "NULL argument");
  ms2[0] = h->last_knn_ms;
  ms2[1] = h->last_total_ms;
  return 0;
}

// One-shot forms: a cached matcher per (device, descriptor width) and calling
// thread, destroyed at thread exit, so repeated calls allocate nothing.
static sfm_matcher* cached_matcher(int32_t device, int32_t desc_bytes, int* rc) {
  struct Cached {
    sfm_matcher* h = nullptr;
    int init(const std::pair<int, int>& key) { return sfm_matcher_create(key.first, key.second, &h); }
    ~Cached() { sfm_matcher_destroy(h); }
  };
  Cached* c = sfm::thread_ctx<Cached>(std::pair<int, int>(device, desc_bytes), rc);
  return c ? c->h : nullptr;
}

int sfm_knn2_hamming(int32_t device, const uint8_t* desc0, int32_t n0, const uint8_t* desc1, int32_t n1,
                     int32_t desc_bytes, int32_t* best_idx, int32_t* best_dist, int32_t* second_idx,
                     int32_t* second_dist) {
  if (n0 < 0 || n1 < 0 || desc_bytes <= 0 || desc_bytes > 512) return fail(SFM_EINVAL, "bad sizes");
  if (n0 == 0) return 0;
  int rc = 0;
  sfm_matcher* h = cached_matcher(device, desc_bytes, &rc);
  if (!h) return rc;
  return sfm_matcher_knn2(h, desc0, n0, desc1, n1, best_idx, best_dist, second_idx, second_dist);
}

int sfm_match_features(int32_t device, const double* pts0, const uint8_t* desc0, int32_t n0, const double* pts1,
                       const uint8_t* desc1, int32_t n1, int32_t desc_bytes, double ratio_test, double min_distance,
                       double max_distance, int32_t* idx0, int32_t* idx1, int32_t* n_matches) {
  if (!n_matches) return fail(SFM_EINVAL, "n_matches is NULL");
  *n_matches = 0;
  if (n0 < 0 || n1 < 0 || desc_bytes <= 0 || desc_bytes > 512) return fail(SFM_EINVAL, "bad sizes");
  if (n0 == 0 || n1 < 2) return 0;  // reference UB with < 2 train rows: no matches
  int rc = 0;
  sfm_matcher* h = cached_matcher(device, desc_bytes, &rc);
  if (!h) return rc;
  return sfm_matcher_match(h, pts0, desc0, n0, pts1, desc1, n1, ratio_test, min_distance, max_distance, idx0, idx1,
                           n_matches);
}

// GeometryUtils::calculateFundamentalMatrix + filterMatches (CSfM.cpp:164-165)
// on host arrays: the kernel body and the host composition of
// sfm_matcher_pair_points (mappoint_kernels.hip), through the cached handle's
// stream and pools.
int sfm_filter_matches(int32_t device, int32_t n, const double* uv0, const double* uv1, const double* X,
                       const double* K9_0, const double* R9_0, const double* t3_0, const double* K9_1,
                       const double* R9_1, const double* t3_1, double max_err, uint8_t* status, double* F9) {
  if (n < 0) return fail(SFM_EINVAL, "negative size");
  if (!K9_0 || !R9_0 || !t3_0 || !K9_1 || !R9_1 || !t3_1) return fail(SFM_EINVAL, "NULL matrix");
  if (n && (!uv0 || !uv1 || !X || !status)) return fail(SFM_EINVAL, "NULL argument");
  if (!std::isfinite(max_err)) return fail(SFM_EINVAL, "non-finite threshold");
  sfm::PairArgs pa;
  if (!sfm::compose_pair(K9_0, R9_0, t3_0, K9_1, R9_1, t3_1, max_err, &pa))
    return fail(SFM_EINVAL, "K must be finite and upper triangular with K[8] = 1, R and t finite");
  if (F9) std::memcpy(F9, pa.F, sizeof(pa.F));
  if (n == 0) return 0;
  int rc = 0;
  sfm_matcher* h = cached_matcher(device, 64, &rc);
  if (!h) return rc;
  if (hipSetDevice(device) != hipSuccess) return fail(SFM_ENODEV, "hipSetDevice failed");
  double* st = pbuf<double>(h, "fin", 7 * size_t(n), &rc);
  double* d = dbuf<double>(h, "dfin", 7 * size_t(n), &rc);
  uint8_t* ds = dbuf<uint8_t>(h, "fst", size_t(n), &rc);
  uint8_t* hs = pbuf<uint8_t>(h, "fsth", size_t(n), &rc);
  if (rc) return rc;
  hipStreamSynchronize(h->stream);
  std::memcpy(st, uv0, sizeof(double) * 2 * size_t(n));
  std::memcpy(st + 2 * size_t(n), uv1, sizeof(double) * 2 * size_t(n));
  std::memcpy(st + 4 * size_t(n), X, sizeof(double) * 3 * size_t(n));
  hipMemcpyAsync(d, st, sizeof(double) * 7 * size_t(n), hipMemcpyHostToDevice, h->stream);
  sfm::launch_filter(h->stream, n, d, d + 2 * size_t(n), d + 4 * size_t(n), pa, ds);
  hipMemcpyAsync(hs, ds, size_t(n), hipMemcpyDeviceToHost, h->stream);
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(SFM_EIO, "filter kernel failed");
  std::memcpy(status, hs, size_t(n));
  return 0;
}

int sfm_representative_descriptors(int32_t device, const uint8_t* desc, const int32_t* row_off, int32_t n_pts,
                                   int32_t desc_bytes, int32_t* best, uint8_t* out) {
  if (n_pts < 0 || desc_bytes <= 0 || desc_bytes > 512) return fail(SFM_EINVAL, "bad sizes");
  if (n_pts == 0) return 0;
  if (!desc || !row_off || !best) return fail(SFM_EINVAL, "NULL argument");
  if (row_off[0] != 0) return fail(SFM_EINVAL, "row_off[0] must be 0");
  for (int32_t i = 0; i < n_pts; ++i)
    if (row_off[i + 1] <= row_off[i])
      return fail(SFM_EINVAL, "every point needs at least one descriptor (the reference reads row -1 otherwise)");
  int rc = 0;
  sfm_matcher* h = cached_matcher(device, desc_bytes, &rc);
  if (!h) return rc;
  if (hipSetDevice(device) != hipSuccess) return fail(SFM_ENODEV, "hipSetDevice failed");
  const int W = h->W;
  const int rows = row_off[n_pts];
  auto* st = pbuf<uint64_t>(h, "in", size_t(rows) * W + size_t(n_pts) + 1, &rc);
  auto* d = dbuf<uint64_t>(h, "din", size_t(rows) * W + size_t(n_pts) + 1, &rc);
  int* r = dbuf<int>(h, "rbest", size_t(n_pts), &rc);
  int* res = pbuf<int>(h, "rres", size_t(n_pts), &rc);
  if (rc) return rc;
  hipStreamSynchronize(h->stream);
  pack_words(desc, rows, desc_bytes, W, st);
  int* so = reinterpret_cast<int*>(st + size_t(rows) * W);
  std::memcpy(so, row_off, (size_t(n_pts) + 1) * sizeof(int));
  hipMemcpyAsync(d, st, (size_t(rows) * W + size_t(n_pts) + 1) * 8, hipMemcpyHostToDevice, h->stream);
  const int* o = reinterpret_cast<const int*>(d + size_t(rows) * W);
  switch (W) {
#define CASE(w) case w: k_repr<w><<<n_pts, 64, 0, h->stream>>>(d, o, n_pts, r); break;
    CASE(1) CASE(2) CASE(4) CASE(8) CASE(16) CASE(32) CASE(64)
#undef CASE
    default: return fail(SFM_EINVAL, "descriptor width must be <= 512 bytes");
  }
  hipMemcpyAsync(res, r, size_t(n_pts) * sizeof(int), hipMemcpyDeviceToHost, h->stream);
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(SFM_EIO, "kernel or copy failed");
  std::memcpy(best, res, size_t(n_pts) * sizeof(int));
  if (out)
    for (int32_t i = 0; i < n_pts; ++i)
      std::memcpy(out + size_t(i) * desc_bytes, desc + (size_t(row_off[i]) + best[i]) * desc_bytes, desc_bytes);
  return 0;
}


// CSfM::tracking's pose step (CSfM.cpp:533-565) as one call: the previous
// frame's keypoints with a map point (prev_pt3d[i] >= 0) matched against the
// whole current frame (matchFeatures(prevIdx, currIdx), CTracker.cpp:368-417),
// their map points and keypoints gathered on the device, and
// cv::solvePnPRansac on them (sfm_pnp_ransac's kernels) -- one upload, one
// download, one synchronisation.  Fewer than min_matches matches: no PnP
// (*found = 0; the caller's lost-tracking branch, CSfM.cpp:545-551).  Outputs:
// *n_matches, the pose (rvec, tvec; zero when not found) and the inliers as
// (current keypoint, map point) pairs.
int sfm_track_pnp(sfm_matcher* h, sfm_map* map, int32_t n_prev, const int32_t* prev_pt3d, double ratio_test,
                  double min_distance, double max_distance, int32_t min_matches, const double* K9, int32_t iterations,
                  double reproj_err, double confidence, double* rvec, double* tvec, int32_t* found,
                  int32_t* n_matches, int32_t capacity, int32_t* inl_kp, int32_t* inl_pt3d, int32_t* n_inliers) {
  SFM_TRACE("sfm_track_pnp");
  if (!h || !map || !found || !n_matches || !n_inliers || !rvec || !tvec || !K9 || !inl_kp || !inl_pt3d)
    return fail(SFM_EINVAL, "NULL argument");
  *found = 0;
  *n_matches = 0;
  *n_inliers = 0;
  for (int i = 0; i < 3; ++i) rvec[i] = tvec[i] = 0.0;
  if (h->frames_pushed < 2) return fail(SFM_EINVAL, "push the previous and the current frame first");
  if (!ok_ratio_window(ratio_test, min_distance, max_distance)) return fail(SFM_EINVAL, "non-finite threshold");
  if (iterations < 0 || iterations > sfm::pnp_max_iters()) return fail(SFM_EINVAL, "bad iterations");
  if (!(confidence > 0.0 && confidence < 1.0)) return fail(SFM_EINVAL, "confidence must lie in (0, 1)");
  const MatchFrame& fp = h->frame[h->cur ^ 1];
  const MatchFrame& fc = h->frame[h->cur];
  if (n_prev != fp.n || (n_prev && !prev_pt3d)) return fail(SFM_EINVAL, "prev_pt3d must hold one entry per previous keypoint");
  int32_t P = 0;
  int mdev = 0;
  const double* X = sfm::map_points_dev(map, &P, &mdev);
  if (mdev != h->device) return fail(SFM_EINVAL, "the map and the matcher are on different devices");
  std::vector<int32_t> pidx;
  pidx.reserve(size_t(n_prev));
  for (int32_t i = 0; i < n_prev; ++i) {
    if (prev_pt3d[i] >= P) return fail(SFM_EINVAL, "map point index out of range");
    if (prev_pt3d[i] >= 0) pidx.push_back(i);
  }
  const int n0 = int(pidx.size()), n1 = fc.n;
  if (n0 == 0 || n1 < 2) return 0;  // (as sfm_matcher_match_subset: no matches)
  if (capacity < n0) return fail(SFM_EINVAL, "capacity below the previous frame's matched keypoints");
  if (hipSetDevice(h->device) != hipSuccess) return fail(SFM_EIO, "hipSetDevice failed");
  int rc = 0;
  const int iters = iterations > 0 ? iterations : 1;
  const size_t n_up = size_t(n0) + size_t(n1) + size_t(n_prev);
  int* ix = pbuf<int>(h, "tidx", n_up, &rc);
  int* dix = dbuf<int>(h, "dtidx", n_up, &rc);
  // result block (ints): count, (pad x3) | found, best, inliers, pad | model
  // (6 doubles) | inliers [n0] | map points [n0] | keypoints [n0]
  const size_t blk = 8 + 12 + 3 * size_t(n0);
  int* dblk = dbuf<int>(h, "tblk", blk, &rc);
  int* hblk = pbuf<int>(h, "tblkh", blk, &rc);
  double* dobj = dbuf<double>(h, "tobj", 5 * size_t(n0), &rc);
  int* dsub = dbuf<int>(h, "tsub", size_t(sfm::pnp_model_size()) * iters, &rc);
  double* dmodel = dbuf<double>(h, "tmodel", 6 * size_t(iters), &rc);
  int* dcnt = dbuf<int>(h, "tcnt", size_t(iters), &rc);
  if (rc) return rc;
  hipStreamSynchronize(h->stream);  // (the pinned stage may feed an earlier copy)
  std::memcpy(ix, pidx.data(), sizeof(int) * size_t(n0));
  for (int i = 0; i < n1; ++i) ix[n0 + i] = i;  // the whole current frame (currIdx)
  if (n_prev) std::memcpy(ix + n0 + n1, prev_pt3d, sizeof(int) * size_t(n_prev));
  hipMemcpyAsync(dix, ix, sizeof(int) * n_up, hipMemcpyHostToDevice, h->stream);
  int* out = nullptr;
  // undistorted positions (CFrame::getPointsAt, CTracker.cpp:375-376)
  if ((rc = run_match_async(h, fp.desc, dix, fp.pts, n0, fc.desc, dix + n0, fc.pts, n1, ratio_test, min_distance,
                            max_distance, &out)))
    return rc;
  int* inl = dblk + 20;
  int* m3 = inl + n0;
  int* kp = m3 + n0;
  k_track_gather<<<(n0 + 255) / 256, 256, 0, h->stream>>>(out, n0, dix, dix + n0 + n1, X, fc.pts, dobj,
                                                          dobj + 3 * size_t(n0), m3, kp, dblk);
  if ((rc = sfm::pnp_ransac_dev(h->stream, dblk, min_matches, dobj, dobj + 3 * size_t(n0), K9, iterations, reproj_err,
                           confidence, dsub, dmodel, dcnt, dblk + 4, inl)))
    return rc;
  hipMemcpyAsync(hblk, dblk, sizeof(int) * blk, hipMemcpyDeviceToHost, h->stream);
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(SFM_EIO, "tracking kernels failed");
  const int m = hblk[0];
  *n_matches = m;
  if (m < min_matches || !hblk[4]) return 0;
  const double* mdl = reinterpret_cast<const double*>(hblk + 8);
  for (int i = 0; i < 3; ++i) { rvec[i] = mdl[i]; tvec[i] = mdl[3 + i]; }
  const int ni = hblk[6];
  const int* hin = hblk + 20;
  for (int i = 0; i < ni; ++i) {
    inl_kp[i] = hblk[20 + 2 * n0 + hin[i]];
    inl_pt3d[i] = hblk[20 + n0 + hin[i]];
  }
  *n_inliers = ni;
  *found = 1;
  return 0;
}
}  // extern "C"
