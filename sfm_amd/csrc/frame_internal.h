// Internal seams of the camera front end (frame_kernels.hip): the detector
// (brisk_kernels.hip), the KLT handle (klt_kernels.hip) and the matcher
// (match_kernels.hip) each own their state; sfm_frame_detect strings them
// together without the frame leaving HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "camera_model.h"

namespace sfm {

// What sfm_frame_detect adds to a detector call.
struct FrameExtras {
  int channels = 1;           // of a host image: 1 (grey) or 3 (CV_RGB2GRAY on the device)
  int stride = 0;             // row stride of a host image in bytes
  LensArgs lens{};            // undistortPoints(_pts_dist, _pts, _K, _d, _Kopt)
  double* pts = nullptr;      // host [capacity][2]: the undistorted positions
  sfm_matcher* mt = nullptr;  // install the result as the matcher's current frame
};

// brisk_kernels.hip.  fx == nullptr: sfm_brisk_detect_describe as it always was.
int brisk_detect_describe_impl(int32_t device, const uint8_t* img, bool img_on_device, int32_t w, int32_t h,
                               int32_t threshold, int32_t octaves, int32_t capacity, float* kps, int32_t* octave,
                               uint8_t* desc, int32_t* n_out, const FrameExtras* fx);

// frame_kernels.hip: launches on stream s, no synchronisation.
void launch_rgb_to_grey(hipStream_t s, const uint8_t* d_rgb, int w, int h, int stride, uint8_t* d_grey);
void launch_undistort_kp3(hipStream_t s, const LensArgs& lens, const float* d_kp3, int n, double* d_out);
// The detector's packed outputs -> the matcher's new current frame (m
// survivors of n keypoints, m as counted by the host from the same keep
// flags).  Returns the matcher's stream in *s; the caller orders its next
// write of the packed buffer after it.
int frame_install(sfm_matcher* mt, int n, int m, const uint8_t* d_desc, const float* d_kp3, const double* d_und,
                  const int32_t* d_keep, hipStream_t* s);

// match_kernels.hip: the slot that becomes the current frame with m
// keypoints (allocated, not yet current) and a scratch of n + 1 ints;
// matcher_install_commit makes it current (the prev/curr swap).
struct MatchSlot {
  uint64_t* desc;
  double* pts;
  double* ptsd;
  int* scratch;
  hipStream_t stream;
};
int matcher_install_begin(sfm_matcher* h, int n, int m, MatchSlot* out);
void matcher_install_commit(sfm_matcher* h, int m);
int matcher_device(const sfm_matcher* h);
int matcher_desc_bytes(const sfm_matcher* h);

// klt_kernels.hip: sfm_klt_push_frame for 1 or 3 channels.
int klt_push_frame_any(sfm_klt_handle* h, const uint8_t* img, int32_t stride, int channels);

}  // namespace sfm
