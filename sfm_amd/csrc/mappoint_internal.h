// Seams of the map-point creation (mappoint_kernels.hip): the kernels and
// the host composition behind sfm_matcher_pair_points,
// sfm_matcher_refind_points, sfm_filter_matches (match_kernels.hip) and
// sfm_map_add_keyframe_rows (map_store.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace sfm {

// What one keyframe pair's kernels read, composed once per call on the host
// (compose_pair) and passed by value as a kernel argument.
struct PairArgs {
  double P0[12], P1[12];  // K [R|t], row-major 3x4
  double F[9];            // K1^-T [t]x R K0^-1, row-major
  double z0[4], z1[4];    // third row of R_i, then t_i[2]: the depth of X in keyframe i
  double max_err;
};

// Host, plain C++, unfused.  false: K is not upper triangular with K[8] = 1
// and non-zero fx, fy (the closed-form inverse needs that), or an input is not
// finite.
bool compose_pair(const double* K0, const double* R0, const double* t0, const double* K1, const double* R1,
                  const double* t1, double max_err, PairArgs* out);

// All launches below: on stream s, no synchronisation.
//
// The matcher's result block `out` ([2 n0 + 1]: query | train | count,
// subset-local) -> per match k < count the triangulated point Xall[k] and the
// keep flag (0 for k >= count); then the kept matches, in match order, into
// the result block: head[0] = kept, head[1] = count, m0 / m1 [n0] the kept
// matches' subset-local indices, X [n0][3] their points.
void launch_pair_points(hipStream_t s, const int* out, int n0, const int* qidx, const int* tidx, const double* pts0,
                        const double* pts1, const PairArgs& a, double* Xall, int* keep, int* src, int* head, int* m0,
                        int* m1, double* X);
// The filter alone on n given matches: status[i] = 1 kept.
void launch_filter(hipStream_t s, int n, const double* uv0, const double* uv1, const double* X, const PairArgs& a,
                   uint8_t* status);
// uv[qidx[i]] = the projection of X[i] (K9: fx, fy, cx, cy read).
void launch_project_rows(hipStream_t s, int n, const int* qidx, const double* X, const double* R9, const double* t3,
                         const double* K9, double* uv);
// dst[k][0..W) = src[rows[k]][0..W)
void launch_copy_desc_rows(hipStream_t s, int n, const int* rows, const uint64_t* src, int W, uint64_t* dst);

}  // namespace sfm
