// Map-point creation of CSfM::mapping (the reference's CSfM.cpp:118-227) on
// the device: per keyframe pair the matcher's matches are triangulated
// (tri_point.h, the arithmetic of sfm_triangulate_points), filtered and
// compacted where they lie, and the new points are projected into the
// keyframes in between for the re-finding (CSfM.cpp:191-221).
//
// The filter is GeometryUtils::calculateFundamentalMatrix + filterMatches as
// read from the call site (CSfM.cpp:164-165; sfm_amd/live.py _filter_matches):
// keep a match iff X is finite, its depth is positive in both keyframes and
// the point-to-epipolar-line distance is <= max_err both ways, with
//   F = K1^-T [t]x R K0^-1,  R = R1 R0^T,  t = t1 - R t0.
// GeometryUtils is in the absent cvUtils library, so PARITY WITH IT IS
// UNPINNED; what is pinned is tests/map_points_ref.py, bit for bit.
//
// Fixed association (this file is compiled with -ffp-contract=off, host and
// device): every 3-term sum is (a b + c d) + e f, a fourth term is added
// last; the host composes F, P0 = K0 [R0|t0] and P1 once per pair in plain
// C++ (compose_pair); the point-creation kernels read them from the call's
// staged table, the filter alone (k_filter) takes them as an argument.  One
// lane per match, no atomics: the keep flags are ordered by compact_keep
// (ordered_compact.h), so the kept matches stay in the matcher's order.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "mappoint_internal.h"
#include "ordered_compact.h"
#include "tri_point.h"

namespace sfm {
namespace {

__host__ __device__ inline double dot3(double a, double b, double c, double d, double e, double f) {
  return (a * b + c * d) + e * f;
}

// keep flag of one match: (u0, v0) in keyframe 0, (u1, v1) in keyframe 1, X
__device__ __forceinline__ bool pair_keep(const PairArgs& a, double u0, double v0, double u1, double v1,
                                          const double X[3]) {
#pragma clang fp contract(off)
  const double* F = a.F;
  // l1 = F h0 (the line of keypoint 0 in image 1), l0 = F^T h1
  const double l1x = (F[0] * u0 + F[1] * v0) + F[2];
  const double l1y = (F[3] * u0 + F[4] * v0) + F[5];
  const double l1z = (F[6] * u0 + F[7] * v0) + F[8];
  const double l0x = (F[0] * u1 + F[3] * v1) + F[6];
  const double l0y = (F[1] * u1 + F[4] * v1) + F[7];
  const double l0z = (F[2] * u1 + F[5] * v1) + F[8];
  const double d1 = fabs((l1x * u1 + l1y * v1) + l1z) / sqrt(l1x * l1x + l1y * l1y);
  const double d0 = fabs((l0x * u0 + l0y * v0) + l0z) / sqrt(l0x * l0x + l0y * l0y);
  const double z0 = dot3(a.z0[0], X[0], a.z0[1], X[1], a.z0[2], X[2]) + a.z0[3];
  const double z1 = dot3(a.z1[0], X[0], a.z1[1], X[1], a.z1[2], X[2]) + a.z1[3];
  const bool fin = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
  // (a NaN distance, F = 0 for two equal poses, fails its comparison)
  return fin && z0 > 0.0 && z1 > 0.0 && d0 <= a.max_err && d1 <= a.max_err;
}

// One lane per match k < count (the count where the matcher left it): both
// keypoints through the subset lists, the point, the flag.
__device__ __forceinline__ void pair_point(const int* __restrict__ out, int n0, const int* __restrict__ qidx,
                                           const int* __restrict__ tidx, const double* __restrict__ pts0,
                                           const double* __restrict__ pts1, const PairArgs& a,
                                           double* __restrict__ Xall, int* __restrict__ keep, int k) {
  if (k >= n0) return;
  if (k >= out[2 * n0]) {
    keep[k] = 0;
    return;
  }
  const size_t r0 = size_t(qidx[out[k]]), r1 = size_t(tidx[out[n0 + k]]);
  const double u0 = pts0[2 * r0], v0 = pts0[2 * r0 + 1], u1 = pts1[2 * r1], v1 = pts1[2 * r1 + 1];
  double X[3];
  tri_point(a.P0, a.P1, u0, v0, u1, v1, X);
  Xall[3 * size_t(k)] = X[0];
  Xall[3 * size_t(k) + 1] = X[1];
  Xall[3 * size_t(k) + 2] = X[2];
  keep[k] = pair_keep(a, u0, v0, u1, v1, X) ? 1 : 0;
}

// item blockIdx.y of a call; its matrices are wave-uniform loads from pa
__global__ __launch_bounds__(256) void k_pair_points_items(const PairItem* __restrict__ items,
                                                           const PairArgs* __restrict__ pa,
                                                           const int* __restrict__ out, const int* __restrict__ idx,
                                                           const int* __restrict__ tidx,
                                                           const double* __restrict__ pts1, double* __restrict__ Xall,
                                                           int* __restrict__ keep) {
  const PairItem& it = items[blockIdx.y];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= it.n0) return;
  pair_point(out + it.out_off, it.n0, idx + it.idx_off, tidx, it.pts, pts1, pa[blockIdx.y], Xall + it.x_off,
             keep + it.idx_off, k);
}

// one workgroup per item: head[1 + item] = its kept count
__global__ __launch_bounds__(1024) void k_compact_keep_items(const PairItem* __restrict__ items,
                                                             const int* __restrict__ keep, int* __restrict__ src,
                                                             int* __restrict__ head) {
  const PairItem& it = items[blockIdx.x];
  compact_keep(it.n0, keep + it.idx_off, src + it.idx_off, head + 1 + blockIdx.x);
}

// the pos-th kept match (src[pos] = the pos-th kept k) into the result block
__device__ __forceinline__ void gather_kept(const int* __restrict__ out, int n0, const int* __restrict__ src,
                                            const double* __restrict__ Xall, int pos, int* __restrict__ m0,
                                            int* __restrict__ m1, double* __restrict__ X) {
  const int k = src[pos];
  m0[pos] = out[k];
  m1[pos] = out[n0 + k];
  X[3 * size_t(pos)] = Xall[3 * size_t(k)];
  X[3 * size_t(pos) + 1] = Xall[3 * size_t(k) + 1];
  X[3 * size_t(pos) + 2] = Xall[3 * size_t(k) + 2];
}

// The pick among a call's B items, one workgroup: every item's match count
// beside its kept count (head: first | kept [B] | matched [B]), the lowest item with a
// kept match -- a min over the lanes' strided items, across the wave by
// shuffles and across the four waves through LDS, so B may exceed a wave --
// and that item's kept matches into the one result block.
__global__ __launch_bounds__(256) void k_pick_first(const PairItem* __restrict__ items, int B,
                                                    const int* __restrict__ out, const int* __restrict__ src,
                                                    const double* __restrict__ Xall, int* __restrict__ head,
                                                    int* __restrict__ m0, int* __restrict__ m1,
                                                    double* __restrict__ X) {
  __shared__ int wave_min[4];
  int best = 0x7fffffff;
  for (int b = threadIdx.x; b < B; b += 256) {
    head[1 + B + b] = out[items[b].out_off + 2 * items[b].n0];
    if (head[1 + b] > 0) best = min(best, b);
  }
  for (int o = 32; o >= 1; o >>= 1) best = min(best, __shfl_xor(best, o));
  if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = best;
  __syncthreads();
  best = min(min(wave_min[0], wave_min[1]), min(wave_min[2], wave_min[3]));
  if (threadIdx.x == 0) head[0] = best == 0x7fffffff ? -1 : best;
  if (best == 0x7fffffff) return;
  const PairItem& it = items[best];
  const int kept = head[1 + best];
  for (int pos = threadIdx.x; pos < kept; pos += 256)
    gather_kept(out + it.out_off, it.n0, src + it.idx_off, Xall + it.x_off, pos, m0, m1, X);
}

__global__ __launch_bounds__(256) void k_filter(int n, const double* __restrict__ uv0, const double* __restrict__ uv1,
                                                const double* __restrict__ X, const PairArgs a,
                                                uint8_t* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double Xi[3] = {X[3 * size_t(i)], X[3 * size_t(i) + 1], X[3 * size_t(i) + 2]};
  status[i] = pair_keep(a, uv0[2 * size_t(i)], uv0[2 * size_t(i) + 1], uv1[2 * size_t(i)], uv1[2 * size_t(i) + 1], Xi);
}

// The formula of map_store.hip's k_project in fixed association, written at
// the query's own row (the matcher reads positions through qidx).
__global__ __launch_bounds__(256) void k_project_rows(int n, const int* __restrict__ qidx, const double* __restrict__ X,
                                                      double r0, double r1, double r2, double r3, double r4, double r5,
                                                      double r6, double r7, double r8, double t0, double t1, double t2,
                                                      double fx, double fy, double cx, double cy,
                                                      double* __restrict__ uv) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = X[3 * size_t(i)], y = X[3 * size_t(i) + 1], z = X[3 * size_t(i) + 2];
  const double c0 = dot3(r0, x, r1, y, r2, z) + t0;
  const double c1 = dot3(r3, x, r4, y, r5, z) + t1;
  const double c2 = dot3(r6, x, r7, y, r8, z) + t2;
  const size_t row = size_t(qidx[i]);
  uv[2 * row] = (c0 / c2) * fx + cx;
  uv[2 * row + 1] = (c1 / c2) * fy + cy;
}

__global__ __launch_bounds__(256) void k_copy_desc_rows(int n, int W, const int* __restrict__ rows,
                                                        const uint64_t* __restrict__ src, uint64_t* __restrict__ dst) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= int64_t(n) * W) return;
  const int k = int(e / W), w = int(e % W);
  dst[e] = src[size_t(rows[k]) * W + w];
}

inline unsigned blocks(int64_t n) { return unsigned((n + 255) / 256); }

// the inverse of an upper-triangular K (fx, skew, cx; fy, cy; 1), closed form
void inv_K(const double* K, double* Ki) {
  const double fx = K[0], s = K[1], cx = K[2], fy = K[4], cy = K[5];
  Ki[0] = 1.0 / fx;
  Ki[1] = -s / (fx * fy);
  Ki[2] = (s * cy - cx * fy) / (fx * fy);
  Ki[3] = 0.0;
  Ki[4] = 1.0 / fy;
  Ki[5] = -cy / fy;
  Ki[6] = 0.0;
  Ki[7] = 0.0;
  Ki[8] = 1.0;
}

// P = K [R|t]
void compose_P(const double* K, const double* R, const double* t, double* P) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) P[4 * i + j] = dot3(K[3 * i], R[j], K[3 * i + 1], R[3 + j], K[3 * i + 2], R[6 + j]);
    P[4 * i + 3] = dot3(K[3 * i], t[0], K[3 * i + 1], t[1], K[3 * i + 2], t[2]);
  }
}

}  // namespace

bool compose_pair(const double* K0, const double* R0, const double* t0, const double* K1, const double* R1,
                  const double* t1, double max_err, PairArgs* out) {
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(K0[i]) || !std::isfinite(K1[i]) || !std::isfinite(R0[i]) || !std::isfinite(R1[i])) return false;
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(t0[i]) || !std::isfinite(t1[i])) return false;
  for (const double* K : {K0, K1})
    if (K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0 || K[0] == 0.0 || K[4] == 0.0) return false;
  compose_P(K0, R0, t0, out->P0);
  compose_P(K1, R1, t1, out->P1);
  double R[9], t[3], E[9], A[9], K0i[9], K1i[9];
  // R = R1 R0^T, t = t1 - R t0
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      R[3 * i + j] = dot3(R1[3 * i], R0[3 * j], R1[3 * i + 1], R0[3 * j + 1], R1[3 * i + 2], R0[3 * j + 2]);
  for (int i = 0; i < 3; ++i) t[i] = t1[i] - dot3(R[3 * i], t0[0], R[3 * i + 1], t0[1], R[3 * i + 2], t0[2]);
  // E = [t]x R, the cross-product matrix written out
  for (int j = 0; j < 3; ++j) {
    E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
    E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
    E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
  }
  inv_K(K0, K0i);
  inv_K(K1, K1i);
  // F = (K1^-T E) K0^-1
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[3 * i + j] = dot3(K1i[i], E[j], K1i[3 + i], E[3 + j], K1i[6 + i], E[6 + j]);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      out->F[3 * i + j] = dot3(A[3 * i], K0i[j], A[3 * i + 1], K0i[3 + j], A[3 * i + 2], K0i[6 + j]);
  for (int j = 0; j < 3; ++j) {
    out->z0[j] = R0[6 + j];
    out->z1[j] = R1[6 + j];
  }
  out->z0[3] = t0[2];
  out->z1[3] = t1[2];
  out->max_err = max_err;
  return true;
}

void launch_pair_points_first(hipStream_t s, const PairItem* items, const PairArgs* pa, int B, int max_n0,
                              const int* out, const int* idx, const int* tidx, const double* pts1, double* Xall,
                              int* keep, int* src, int* head, int* m0, int* m1, double* X) {
  k_pair_points_items<<<dim3(blocks(max_n0), B), 256, 0, s>>>(items, pa, out, idx, tidx, pts1, Xall, keep);
  k_compact_keep_items<<<B, 1024, 0, s>>>(items, keep, src, head);
  k_pick_first<<<1, 256, 0, s>>>(items, B, out, src, Xall, head, m0, m1, X);
}

void launch_filter(hipStream_t s, int n, const double* uv0, const double* uv1, const double* X, const PairArgs& a,
                   uint8_t* status) {
  k_filter<<<blocks(n), 256, 0, s>>>(n, uv0, uv1, X, a, status);
}

void launch_project_rows(hipStream_t s, int n, const int* qidx, const double* X, const double* R9, const double* t3,
                         const double* K9, double* uv) {
  k_project_rows<<<blocks(n), 256, 0, s>>>(n, qidx, X, R9[0], R9[1], R9[2], R9[3], R9[4], R9[5], R9[6], R9[7], R9[8],
                                           t3[0], t3[1], t3[2], K9[0], K9[4], K9[2], K9[5], uv);
}

void launch_copy_desc_rows(hipStream_t s, int n, const int* rows, const uint64_t* src, int W, uint64_t* dst) {
  k_copy_desc_rows<<<blocks(int64_t(n) * W), 256, 0, s>>>(n, W, rows, src, dst);
}

}  // namespace sfm
