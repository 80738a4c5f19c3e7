// The lens model of CFrame (cv::undistortPoints, CFrame.cpp:203-227), shared
// by the host (camera.cpp: getOptimalNewCameraMatrix) and the device
// (frame_kernels.hip).  OpenCV is not available to this project: this is its
// restatement of OpenCV 3.0's arithmetic, parity with OpenCV unpinned
// (DESIGN.md); tests/camera_ref.py restates the same operations in numpy and
// both sides are compared bit for bit, so every expression below keeps its
// operation order and is compiled with -ffp-contract=off.
#pragma once
#include <cstdint>
#include "../../include/sfm_amd.h"

#if defined(__HIPCC__)
#define SFM_HD __host__ __device__
#else
#define SFM_HD
#endif

namespace sfm {

// fx, fy, cx, cy of K and of P, and d = k1 k2 p1 p2 k3 k4 k5 k6 (missing: 0)
struct LensArgs {
  double fx, fy, cx, cy;
  double nfx, nfy, ncx, ncy;
  double d[8];
};

inline bool lens_nd_ok(int32_t n_d) { return n_d == 0 || n_d == 4 || n_d == 5 || n_d == 8; }

inline LensArgs lens_args(const sfm_camera& c) {
  LensArgs a;
  a.fx = c.K9[0]; a.fy = c.K9[4]; a.cx = c.K9[2]; a.cy = c.K9[5];
  a.nfx = c.Kopt9[0]; a.nfy = c.Kopt9[4]; a.ncx = c.Kopt9[2]; a.ncy = c.Kopt9[5];
  for (int i = 0; i < 8; ++i) a.d[i] = i < c.n_d ? c.d[i] : 0.0;
  return a;
}

// Pixel (u, v) of K's image -> normalised undistorted (x, y): five fixed-point
// iterations, no convergence test.
SFM_HD inline void undistort_normalised(const LensArgs& L, double u, double v, double& x, double& y) {
  const double k1 = L.d[0], k2 = L.d[1], p1 = L.d[2], p2 = L.d[3], k3 = L.d[4], k4 = L.d[5], k5 = L.d[6],
               k6 = L.d[7];
  const double x0 = (u - L.cx) / L.fx, y0 = (v - L.cy) / L.fy;
  x = x0;
  y = y0;
  for (int it = 0; it < 5; ++it) {
    const double r2 = x * x + y * y;
    const double icd = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
    const double dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
    const double dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
    x = (x0 - dx) * icd;
    y = (y0 - dy) * icd;
  }
}

// cv::undistortPoints(src, dst, K, d, P) for one point.
SFM_HD inline void undistort_pixel(const LensArgs& L, double u, double v, double& uo, double& vo) {
  double x, y;
  undistort_normalised(L, u, v, x, y);
  uo = x * L.nfx + L.ncx;
  vo = y * L.nfy + L.ncy;
}

}  // namespace sfm
