// sfm_camera_init: the camera of CSfM(K, imSize, d) with
// _Kopt = getOptimalNewCameraMatrix(_K, _d, _imSize, 0) (CFrame.cpp:33).
// Host only (called once per camera; works without a GPU).  OpenCV 3.0's
// arithmetic as restated in the issue and in tests/camera_ref.py (parity with
// OpenCV unpinned): alpha = 0, default newImgSize, no centred
// principal point.
#include <cmath>
#include <cstdint>
#include <string>
#include "camera_model.h"
#include "sfm_error.h"

extern "C" int sfm_camera_init(sfm_camera* cam, const double* K9, const double* d, int32_t n_d, int32_t width,
                               int32_t height) {
  if (!cam || !K9) return fail(SFM_EINVAL, "NULL argument");
  if (!sfm::lens_nd_ok(n_d)) return fail(SFM_EINVAL, "n_d must be 0, 4, 5 or 8");
  if (n_d && !d) return fail(SFM_EINVAL, "d is NULL");
  if (width < 2 || height < 2) return fail(SFM_EINVAL, "image size must be at least 2 x 2");
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(K9[i])) return fail(SFM_EINVAL, "K is not finite");
  for (int i = 0; i < n_d; ++i)
    if (!std::isfinite(d[i])) return fail(SFM_EINVAL, "d is not finite");
  if (!(K9[0] > 0.0) || !(K9[4] > 0.0)) return fail(SFM_EINVAL, "fx and fy must be positive");
  for (int i = 0; i < 9; ++i) cam->K9[i] = K9[i];
  for (int i = 0; i < 8; ++i) cam->d[i] = i < n_d ? d[i] : 0.0;
  cam->n_d = n_d;
  cam->width = width;
  cam->height = height;
  cam->reserved = 0;
  for (int i = 0; i < 9; ++i) cam->Kopt9[i] = (i % 4 == 0) ? 1.0 : 0.0;
  const sfm::LensArgs L = sfm::lens_args(*cam);
  // icvGetRectangles: the 9 x 9 grid (float32), undistorted to normalised
  // coordinates (float32); the inner rectangle in float32
  const float inf = INFINITY;
  float X0 = -inf, X1 = inf, Y0 = -inf, Y1 = inf;
  for (int j = 0; j < 9; ++j)
    for (int i = 0; i < 9; ++i) {
      const float u = float(i) * float(width) / 8.0f, v = float(j) * float(height) / 8.0f;
      double xd, yd;
      sfm::undistort_normalised(L, double(u), double(v), xd, yd);
      const float x = float(xd), y = float(yd);
      if (i == 0) X0 = std::fmax(X0, x);
      if (i == 8) X1 = std::fmin(X1, x);
      if (j == 0) Y0 = std::fmax(Y0, y);
      if (j == 8) Y1 = std::fmin(Y1, y);
    }
  const float rw = X1 - X0, rh = Y1 - Y0;
  if (!(rw > 0.0f) || !(rh > 0.0f) || !std::isfinite(rw) || !std::isfinite(rh))
    return fail(SFM_EINVAL, "the lens leaves no valid rectangle (getOptimalNewCameraMatrix)");
  const double fx = double(width - 1) / double(rw), fy = double(height - 1) / double(rh);
  cam->Kopt9[0] = fx;
  cam->Kopt9[4] = fy;
  cam->Kopt9[2] = -fx * double(X0);
  cam->Kopt9[5] = -fy * double(Y0);
  return 0;
}
