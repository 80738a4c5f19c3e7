// cv::triangulatePoints (OpenCV 3.0 cvTriangulatePoints) for one point seen
// at (xa, ya) through Pa and at (xb, yb) through Pb (row-major 3x4): the 4x4
// system  x P_3 - P_1,  y P_3 - P_2  of both views, its right singular vector
// of the smallest singular value (cv::SVD, cv_linalg.h), the homogeneous
// division.  Shared by tri_kernels.hip (sfm_triangulate_points) and
// init_kernels.hip (the vote and the triangulation of sfm_two_view_init).
// Returns the homogeneous coordinate that X was divided by.
#pragma once
#include "cv_linalg.h"

namespace sfm {
namespace {

__device__ __forceinline__ double tri_point(const double* __restrict__ Pa, const double* __restrict__ Pb, double xa,
                                            double ya, double xb, double yb, double X[3]) {
  double A[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    A[0][k] = xa * Pa[8 + k] - Pa[k];
    A[1][k] = ya * Pa[8 + k] - Pa[4 + k];
    A[2][k] = xb * Pb[8 + k] - Pb[k];
    A[3][k] = yb * Pb[8 + k] - Pb[4 + k];
  }
  double U[4][4], w[4], Vt[4][4];
  cv_svd<4, 4>(A, U, w, Vt);
  const double h = Vt[3][3];
  X[0] = Vt[3][0] / h;
  X[1] = Vt[3][1] / h;
  X[2] = Vt[3][2] / h;
  return h;
}

}  // namespace
}  // namespace sfm
