// Camera front end on the device: what CFrame does to every frame before the
// tracker sees it.
//
//   k_rgb_to_grey       CFrame::setFrame: cvtColor(.., CV_RGB2GRAY)
//                       (/root/reference/CFrame.cpp:156-164)
//   k_undistort_points  CFrame::setKeyPoints: undistortPoints(_pts_dist, _pts,
//                       _K, _d, _Kopt)  (CFrame.cpp:203-227)
//   k_frame_install     the detector's packed outputs -> the matcher's
//                       resident current frame, device to device
//
// OpenCV is not available to this project: the arithmetic is its restatement
// of OpenCV 3.0 (camera_model.h, tests/camera_ref.py), bit for bit against
// that restatement, parity with OpenCV unpinned.
//
// All three are memory-bound and tiny next to the detector; what they buy is
// the copies they remove: a colour frame is uploaded once and converted into
// its consumer's buffer (the KLT level-0 slot or the detector's layer 0), and
// a detected frame reaches the matcher without the host compacting,
// re-packing and re-uploading what the detector has just downloaded.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include "sfm_trace.h"
#include "../../include/sfm_amd.h"
#include "frame_internal.h"
#include "klt_internal.h"
#include "ordered_compact.h"
#include "dev_mem.h"

namespace sfm {
namespace {

// g = (c0*4899 + c1*9617 + c2*1868 + 8192) >> 14; c0 is the first channel in
// memory (the reference hands VideoCapture's BGR frames to CV_RGB2GRAY: the
// call is reproduced as made).
__device__ __forceinline__ unsigned grey_of(unsigned c0, unsigned c1, unsigned c2) {
  return (c0 * 4899u + c1 * 9617u + c2 * 1868u + 8192u) >> 14;
}

// One lane, four pixels: three dword loads, one dword store.  Rows start at
// any byte (stride and width are the caller's), so the dwords go through
// memcpy, which is one unaligned global load / store each on gfx950.  The
// w % 4 pixels of a row's tail go byte by byte: nothing is read past the
// row's 3 * w bytes and nothing written past its w.
__global__ __launch_bounds__(256) void k_rgb_to_grey(const uint8_t* __restrict__ rgb, int w, int h, int stride,
                                                     uint8_t* __restrict__ grey) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  const int x = 4 * q;
  if (x >= w || y >= h) return;
  const uint8_t* s = rgb + size_t(y) * stride + 3 * size_t(x);
  uint8_t* d = grey + size_t(y) * w + x;
  if (x + 4 <= w) {
    uint32_t a, b, c;
    __builtin_memcpy(&a, s, 4);
    __builtin_memcpy(&b, s + 4, 4);
    __builtin_memcpy(&c, s + 8, 4);
    const unsigned g0 = grey_of(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
    const unsigned g1 = grey_of(a >> 24, b & 255u, (b >> 8) & 255u);
    const unsigned g2 = grey_of((b >> 16) & 255u, b >> 24, c & 255u);
    const unsigned g3 = grey_of((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
    const uint32_t o = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    __builtin_memcpy(d, &o, 4);
  } else {
    for (int k = 0; x + k < w; ++k) d[k] = uint8_t(grey_of(s[3 * k], s[3 * k + 1], s[3 * k + 2]));
  }
}

// One lane per point, fp64.  kKp3: the detector's (x, y, size) float triples
// (float -> double is exact); otherwise double[n][2].
template <bool kKp3>
__global__ __launch_bounds__(256) void k_undistort_points(LensArgs L, const void* __restrict__ src, int n,
                                                          double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double u, v;
  if (kKp3) {
    const float* p = static_cast<const float*>(src) + 3 * size_t(i);
    u = double(p[0]);
    v = double(p[1]);
  } else {
    const double2 p = static_cast<const double2*>(src)[i];
    u = p.x;
    v = p.y;
  }
  double uo, vo;
  undistort_pixel(L, u, v, uo, vo);
  reinterpret_cast<double2*>(out)[i] = make_double2(uo, vo);
}

// Survivor `pos` of BRISK's order is keypoint src[pos] (k_compact_keep on the
// descriptor's keep flags).  Eight lanes per survivor copy its eight
// descriptor words (the bytes as they lie, which is pack_words' order for a
// 64-byte descriptor); the first two also write the undistorted position and
// the distorted one as doubles: [desc m*8 | pts 2m | ptsd 2m], MatchFrame.
__global__ __launch_bounds__(256) void k_frame_install(int m, const int* __restrict__ src,
                                                       const uint64_t* __restrict__ desc_in,
                                                       const float* __restrict__ kp3,
                                                       const double* __restrict__ und, uint64_t* __restrict__ desc,
                                                       double* __restrict__ pts, double* __restrict__ ptsd) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int pos = t >> 3, wd = t & 7;
  if (pos >= m) return;
  const int k = src[pos];
  desc[size_t(pos) * 8 + wd] = desc_in[size_t(k) * 8 + wd];
  if (wd == 0) {
    reinterpret_cast<double2*>(pts)[pos] = reinterpret_cast<const double2*>(und)[k];
  } else if (wd == 1) {
    reinterpret_cast<double2*>(ptsd)[pos] = make_double2(double(kp3[3 * size_t(k)]), double(kp3[3 * size_t(k) + 1]));
  }
}

int check_camera(const sfm_camera* cam) {
  if (!cam) return fail(SFM_EINVAL, "cam is NULL");
  if (!lens_nd_ok(cam->n_d)) return fail(SFM_EINVAL, "n_d must be 0, 4, 5 or 8");
  if (cam->width < 2 || cam->height < 2) return fail(SFM_EINVAL, "image size must be at least 2 x 2");
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(cam->K9[i]) || !std::isfinite(cam->Kopt9[i])) return fail(SFM_EINVAL, "K or Kopt is not finite");
  for (int i = 0; i < cam->n_d; ++i)
    if (!std::isfinite(cam->d[i])) return fail(SFM_EINVAL, "d is not finite");
  if (!(cam->K9[0] > 0.0) || !(cam->K9[4] > 0.0)) return fail(SFM_EINVAL, "fx and fy must be positive");
  return 0;
}

}  // namespace

void launch_rgb_to_grey(hipStream_t s, const uint8_t* d_rgb, int w, int h, int stride, uint8_t* d_grey) {
  const int quads = (w + 3) / 4;
  const int bx = quads >= 256 ? 256 : 64;
  dim3 g(unsigned((quads + bx - 1) / bx), unsigned(h));
  k_rgb_to_grey<<<g, bx, 0, s>>>(d_rgb, w, h, stride, d_grey);
}

void launch_undistort_kp3(hipStream_t s, const LensArgs& lens, const float* d_kp3, int n, double* d_out) {
  if (n > 0) k_undistort_points<true><<<(n + 255) / 256, 256, 0, s>>>(lens, d_kp3, n, d_out);
}

int frame_install(sfm_matcher* mt, int n, int m, const uint8_t* d_desc, const float* d_kp3, const double* d_und,
                  const int32_t* d_keep, hipStream_t* s) {
  MatchSlot slot;
  if (int rc = matcher_install_begin(mt, n, m, &slot)) return rc;
  *s = slot.stream;
  if (m > 0) {
    k_compact_keep<<<1, 1024, 0, slot.stream>>>(n, d_keep, slot.scratch, slot.scratch + n);
    k_frame_install<<<(8 * m + 255) / 256, 256, 0, slot.stream>>>(m, slot.scratch,
                                                                  reinterpret_cast<const uint64_t*>(d_desc), d_kp3,
                                                                  d_und, slot.desc, slot.pts, slot.ptsd);
    if (hipGetLastError() != hipSuccess) return fail(SFM_EIO, "frame install launch failed");
  }
  matcher_install_commit(mt, m);
  return 0;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_undistort_points(int32_t device, const sfm_camera* cam, int32_t n, const double* pts_dist, double* pts) {
  SFM_TRACE("sfm_undistort_points");
  if (int rc = check_camera(cam)) return rc;
  if (n < 0 || (n > 0 && (!pts_dist || !pts))) return fail(SFM_EINVAL, "bad point arguments");
  if (n == 0) return 0;
  if (hipSetDevice(device) != hipSuccess) return fail(SFM_ENODEV, "hipSetDevice failed");
  const size_t bytes = 16 * size_t(n);
  DevArr<double> d_in;
  if (d_in.reserve(2 * bytes, 2 * bytes, nullptr)) return fail(SFM_ENOMEM, "hipMalloc failed (undistort)");
  double* d_out = d_in + 2 * size_t(n);
  bool ok = hipMemcpy(d_in, pts_dist, bytes, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    k_undistort_points<false><<<(n + 255) / 256, 256>>>(lens_args(*cam), d_in, n, d_out);
    ok = hipGetLastError() == hipSuccess && hipMemcpy(pts, d_out, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  }
  return ok ? 0 : fail(SFM_EIO, "copy or kernel failed (undistort)");
}

int sfm_rgb_to_grey(int32_t device, const uint8_t* rgb, int32_t w, int32_t h, int32_t stride, uint8_t* grey) {
  SFM_TRACE("sfm_rgb_to_grey");
  if (!rgb || !grey) return fail(SFM_EINVAL, "NULL argument");
  if (w < 1 || h < 1 || int64_t(stride) < 3 * int64_t(w)) return fail(SFM_EINVAL, "bad sizes (stride >= 3 * w)");
  if (hipSetDevice(device) != hipSuccess) return fail(SFM_ENODEV, "hipSetDevice failed");
  const size_t in_bytes = size_t(h - 1) * stride + 3 * size_t(w), out_bytes = size_t(w) * h;
  DevArr<uint8_t> d_rgb, d_grey;
  if (d_rgb.reserve(in_bytes, in_bytes, nullptr) || d_grey.reserve(out_bytes, out_bytes, nullptr))
    return fail(SFM_ENOMEM, "hipMalloc failed (grey conversion)");
  bool ok = hipMemcpy(d_rgb, rgb, in_bytes, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    launch_rgb_to_grey(nullptr, d_rgb, w, h, stride, d_grey);
    ok = hipGetLastError() == hipSuccess && hipMemcpy(grey, d_grey, out_bytes, hipMemcpyDeviceToHost) == hipSuccess;
  }
  return ok ? 0 : fail(SFM_EIO, "copy or kernel failed (grey conversion)");
}

int sfm_frame_detect(sfm_matcher* mt, sfm_klt_handle* klt, const uint8_t* img, int32_t channels, int32_t stride,
                     const sfm_camera* cam, int32_t threshold, int32_t octaves, int32_t capacity, float* kps,
                     int32_t* octave, uint8_t* desc, double* pts, int32_t* n_out) {
  SFM_TRACE("sfm_frame_detect");
  if (!n_out) return fail(SFM_EINVAL, "n_out is NULL");
  *n_out = 0;
  if (int rc = check_camera(cam)) return rc;
  if (!img) return fail(SFM_EINVAL, "img is NULL");
  if (channels != 1 && channels != 3) return fail(SFM_EINVAL, "channels must be 1 or 3");
  const int w = cam->width, h = cam->height;
  if (int64_t(stride) < int64_t(channels) * w) return fail(SFM_EINVAL, "stride < channels * width");
  if (capacity < 0 || (capacity && (!kps || !octave || !pts))) return fail(SFM_EINVAL, "NULL argument");
  int device = 0;
  KltFrame kf{};
  if (mt) {
    if (matcher_desc_bytes(mt) != 64) return fail(SFM_EINVAL, "the matcher's descriptors are not 64 bytes");
    if (!desc) return fail(SFM_EINVAL, "the hand-off to a matcher needs descriptors");
    device = matcher_device(mt);
  }
  FrameExtras fx;
  fx.channels = channels;
  fx.stride = stride;
  fx.lens = lens_args(*cam);
  fx.pts = pts;
  fx.mt = mt;
  if (klt) {
    // CTracker::setCurrentFrame: the frame becomes the handle's current one
    // (pyramid and all); BRISK then runs on that resident frame
    const int kw = sfm_internal_klt_size(klt, &kf);
    if (kw != 0) return kw;
    if (kf.w != w || kf.h != h) return fail(SFM_EINVAL, "the KLT handle's frame size is not the camera's");
    if (mt && kf.device != device) return fail(SFM_EINVAL, "matcher and KLT handle are on different devices");
    device = kf.device;
    if (int rc = klt_push_frame_any(klt, img, stride, channels)) return rc;
    if (int rc = sfm_internal_klt_frame(klt, &kf)) return rc;
    fx.channels = 1;
    fx.stride = w;
    return brisk_detect_describe_impl(device, kf.img, true, w, h, threshold, octaves, capacity, kps, octave, desc,
                                      n_out, &fx);
  }
  if (!mt && hipGetDevice(&device) != hipSuccess) return fail(SFM_ENODEV, "no HIP device");
  return brisk_detect_describe_impl(device, img, false, w, h, threshold, octaves, capacity, kps, octave, desc, n_out,
                                    &fx);
}

}  // extern "C"
