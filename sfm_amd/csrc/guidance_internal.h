// Shared between guidance_kernels.hip (device stages, the handle) and
// guidance_host.cpp (hull + minAreaRect, host only).
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/sfm_amd.h"

namespace sfm {
struct GPoint {
  int32_t x, y;
};
// Strict hull from the smallest (x, y) point, clockwise with y pointing up.
std::vector<GPoint> guidance_convex_hull(std::vector<GPoint> pts);
// cv::minAreaRect: cx cy w h angle (degrees).
void guidance_min_area_rect(const std::vector<GPoint>& pts, float box5[5]);
}  // namespace sfm
