// Seams of the map-point creation (mappoint_kernels.hip): the kernels and
// the host composition behind sfm_matcher_pair_points and
// sfm_matcher_pair_points_first (one path, pair_points_run),
// sfm_matcher_refind_points, sfm_filter_matches (match_kernels.hip) and
// sfm_map_add_keyframe_rows (map_store.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace sfm {

// What one keyframe pair's kernels read, composed once per pair on the host
// (compose_pair): staged with the item table for the point creation, passed
// by value as a kernel argument to the filter alone (launch_filter).
struct PairArgs {
  double P0[12], P1[12];  // K [R|t], row-major 3x4
  double F[9];            // K1^-T [t]x R K0^-1, row-major
  double z0[4], z1[4];    // third row of R_i, then t_i[2]: the depth of X in keyframe i
  double max_err;
};

// One keyframe pair of a point-creation call (sfm_matcher_pair_points: one
// item; sfm_matcher_pair_points_first: n_pairs): the older keyframe's rows and
// where this pair's pieces lie in the call's buffers.  The table is
// device-resident, staged with the index lists; the new keyframe's side (its
// rows, idx1, n1) is common to all items.
struct PairItem {
  const uint64_t* desc;  // the older keyframe's descriptor words [.][W]
  const double* pts;     // ... and positions [.][2]
  int n0;                // rows of this item
  int idx_off;           // idx0 list in the staged index lists; also slot / keep / src (one int per row)
  int out_off;           // the matcher's block out [2 n0 + 1]
  int pad;
  long long part_off;    // partial 2-NN keys [nslice][n0][2]
  long long key_off;     // key / first [n1]
  long long x_off;       // Xall [n0][3]
};

// Host, plain C++, unfused.  false: K is not upper triangular with K[8] = 1
// and non-zero fx, fy (the closed-form inverse needs that), or an input is not
// finite.
bool compose_pair(const double* K0, const double* R0, const double* t0, const double* K1, const double* R1,
                  const double* t1, double max_err, PairArgs* out);

// All launches below: on stream s, no synchronisation.
//
// The tail of a point-creation call of B items (B = 1: one keyframe pair).
// Per item b the matcher's result block out + out_off ([2 n0 + 1]: query |
// train | count, subset-local) -> per match k < count the triangulated point
// Xall[x_off + k] through pa[b] and the keep flag (0 for k >= count), then
// their ordered compaction (src + idx_off; head[1 + b] = kept); then the
// pick: head[1 + B + b] = matched, head[0] = the lowest b with kept > 0 (-1:
// none) and that item's kept matches, in match order, in m0 / m1 (subset-local
// indices) and X (their points).  Three launches whatever B; max_n0 = the
// longest item.
void launch_pair_points_first(hipStream_t s, const PairItem* items, const PairArgs* pa, int B, int max_n0,
                              const int* out, const int* idx, const int* tidx, const double* pts1, double* Xall,
                              int* keep, int* src, int* head, int* m0, int* m1, double* X);
// The filter alone on n given matches: status[i] = 1 kept.
void launch_filter(hipStream_t s, int n, const double* uv0, const double* uv1, const double* X, const PairArgs& a,
                   uint8_t* status);
// uv[qidx[i]] = the projection of X[i] (K9: fx, fy, cx, cy read).
void launch_project_rows(hipStream_t s, int n, const int* qidx, const double* X, const double* R9, const double* t3,
                         const double* K9, double* uv);
// dst[k][0..W) = src[rows[k]][0..W)
void launch_copy_desc_rows(hipStream_t s, int n, const int* rows, const uint64_t* src, int W, uint64_t* dst);

// CMap::getRepresentativeDescriptors' choice (CMap.cpp:345-381) for k_repr
// (match_kernels.hip: contiguous rows) and k_map_repr (map_store.hip: rows by
// CSR).  One wave per point, lane l: of the point's k rows (row(r): row r's W
// words) the one with the smallest sum of Hamming distances to all k, the
// first on ties (integer sums).  Every lane returns it; k = 0: -1.
template <int W, typename Row>
__device__ inline int repr_row(int k, int l, Row row) {
  unsigned long long key = ~0ull;  // (sum << 32 | row): the min is the first minimal row
  for (int r = l; r - l < k; r += 64) {  // lane l owns rows l, l + 64, ...
    uint64_t x[W];
    const uint64_t* xr = row(r < k ? r : 0);
#pragma unroll
    for (int w = 0; w < W; ++w) x[w] = xr[w];
    unsigned int sum = 0;
    for (int q = 0; q < k; ++q) {
      const uint64_t* y = row(q);  // wave-uniform: one line per instruction
#pragma unroll
      for (int w = 0; w < W; ++w) sum += __popcll(x[w] ^ y[w]);
    }
    if (r < k) key = min(key, (static_cast<unsigned long long>(sum) << 32) | unsigned(r));
  }
  for (int o = 32; o >= 1; o >>= 1) key = min(key, static_cast<unsigned long long>(__shfl_xor(key, o)));
  return int(key & 0xffffffffu);
}

}  // namespace sfm
