// Host tail of the scan guidance (CScanGuidance.cpp:99): cv::minAreaRect of
// integer points -- the convex hull, then OpenCV 3.0's rotatingCalipers(..,
// CALIPERS_MINAREARECT) in float32 -- as restated in tests/guidance_ref.py
// (parity with OpenCV unpinned).  Host only: sfm_min_area_rect and
// sfm_guidance_default_options work without a GPU.  Built unfused, as the
// numpy restatement rounds.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include "guidance_internal.h"
#include "sfm_error.h"

namespace sfm {

// Strict hull (no collinear vertex) from the lexicographically smallest
// (x, y) point, clockwise in a frame whose y axis points up.
std::vector<GPoint> guidance_convex_hull(std::vector<GPoint> p) {
  std::sort(p.begin(), p.end(), [](const GPoint& a, const GPoint& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
  p.erase(std::unique(p.begin(), p.end(), [](const GPoint& a, const GPoint& b) { return a.x == b.x && a.y == b.y; }),
          p.end());
  const size_t n = p.size();
  if (n <= 1) return p;
  auto cross = [](const GPoint& a, const GPoint& b, const GPoint& c) {
    return (int64_t(b.x) - a.x) * (int64_t(c.y) - a.y) - (int64_t(b.y) - a.y) * (int64_t(c.x) - a.x);
  };
  std::vector<GPoint> h(2 * n);
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) {  // lower chain
    while (k >= 2 && cross(h[k - 2], h[k - 1], p[i]) <= 0) --k;
    h[k++] = p[i];
  }
  for (size_t i = n - 1, t = k + 1; i > 0; --i) {  // upper chain
    while (k >= t && cross(h[k - 2], h[k - 1], p[i - 1]) <= 0) --k;
    h[k++] = p[i - 1];
  }
  h.resize(k - 1);  // counter-clockwise, h[0] the smallest point
  std::reverse(h.begin() + 1, h.end());
  return h;
}

namespace {

void rotating_calipers(const std::vector<GPoint>& hull, float out[6]) {
  const int n = int(hull.size());
  std::vector<float> px(n), py(n), vx(n), vy(n), inv(n);
  for (int i = 0; i < n; ++i) {
    px[i] = float(hull[i].x);
    py[i] = float(hull[i].y);
  }
  int left = 0, bottom = 0, right = 0, top = 0;
  float left_x = px[0], right_x = px[0], top_y = py[0], bottom_y = py[0];
  for (int i = 0; i < n; ++i) {
    if (px[i] < left_x) left_x = px[i], left = i;
    if (px[i] > right_x) right_x = px[i], right = i;
    if (py[i] > top_y) top_y = py[i], top = i;
    if (py[i] < bottom_y) bottom_y = py[i], bottom = i;
    const int j = i + 1 < n ? i + 1 : 0;
    const double dx = double(px[j]) - double(px[i]), dy = double(py[j]) - double(py[i]);
    vx[i] = float(dx);
    vy[i] = float(dy);
    inv[i] = float(1. / std::sqrt(dx * dx + dy * dy));
  }
  float orientation = 0.f;
  {
    double ax = vx[n - 1], ay = vy[n - 1];
    for (int i = 0; i < n; ++i) {
      const double bx = vx[i], by = vy[i];
      const double convexity = ax * by - ay * bx;
      if (convexity != 0) {
        orientation = convexity > 0 ? 1.f : -1.f;
        break;
      }
      ax = bx;
      ay = by;
    }
  }
  float base_a = orientation, base_b = 0.f;
  int seq[4] = {bottom, right, top, left};
  float minarea = FLT_MAX;
  int b_left = 0, b_bottom = 0;
  float b_a = 0.f, b_b = 0.f, b_width = 0.f, b_height = 0.f;
  for (int k = 0; k < n; ++k) {
    const float dp0 = base_a * vx[seq[0]] + base_b * vy[seq[0]];
    const float dp1 = -base_b * vx[seq[1]] + base_a * vy[seq[1]];
    const float dp2 = -base_a * vx[seq[2]] - base_b * vy[seq[2]];
    const float dp3 = base_b * vx[seq[3]] - base_a * vy[seq[3]];
    float maxcos = dp0 * inv[seq[0]];
    int main_element = 0;
    float cosalpha = dp1 * inv[seq[1]];
    if (cosalpha > maxcos) main_element = 1, maxcos = cosalpha;
    cosalpha = dp2 * inv[seq[2]];
    if (cosalpha > maxcos) main_element = 2, maxcos = cosalpha;
    cosalpha = dp3 * inv[seq[3]];
    if (cosalpha > maxcos) main_element = 3, maxcos = cosalpha;
    const int pindex = seq[main_element];
    const float lead_x = vx[pindex] * inv[pindex], lead_y = vy[pindex] * inv[pindex];
    switch (main_element) {
      case 0: base_a = lead_x, base_b = lead_y; break;
      case 1: base_a = lead_y, base_b = -lead_x; break;
      case 2: base_a = -lead_x, base_b = -lead_y; break;
      default: base_a = -lead_y, base_b = lead_x; break;
    }
    seq[main_element] = seq[main_element] + 1 == n ? 0 : seq[main_element] + 1;
    float dx = px[seq[1]] - px[seq[3]], dy = py[seq[1]] - py[seq[3]];
    const float width = dx * base_a + dy * base_b;
    dx = px[seq[2]] - px[seq[0]];
    dy = py[seq[2]] - py[seq[0]];
    const float height = -dx * base_b + dy * base_a;
    const float area = width * height;
    if (area <= minarea) {
      minarea = area;
      b_left = seq[3];
      b_a = base_a;
      b_width = width;
      b_b = base_b;
      b_height = height;
      b_bottom = seq[0];
    }
  }
  const float A1 = b_a, B1 = b_b, A2 = -b_b, B2 = b_a;
  const float C1 = A1 * px[b_left] + py[b_left] * B1;
  const float C2 = A2 * px[b_bottom] + py[b_bottom] * B2;
  const float idet = 1.f / (A1 * B2 - A2 * B1);
  out[0] = (C1 * B2 - C2 * B1) * idet;
  out[1] = (A1 * C2 - A2 * C1) * idet;
  out[2] = A1 * b_width;
  out[3] = B1 * b_width;
  out[4] = A2 * b_height;
  out[5] = B2 * b_height;
}

}  // namespace

void guidance_min_area_rect(const std::vector<GPoint>& pts, float box5[5]) {
  const std::vector<GPoint> hull = guidance_convex_hull(pts);
  const size_t n = hull.size();
  float cx = 0.f, cy = 0.f, w = 0.f, h = 0.f, angle = 0.f;
  if (n > 2) {
    float o[6];
    rotating_calipers(hull, o);
    cx = o[0] + (o[2] + o[4]) * 0.5f;
    cy = o[1] + (o[3] + o[5]) * 0.5f;
    w = float(std::sqrt(double(o[2]) * o[2] + double(o[3]) * o[3]));
    h = float(std::sqrt(double(o[4]) * o[4] + double(o[5]) * o[5]));
    angle = float(std::atan2(double(o[3]), double(o[2])));
  } else if (n == 2) {
    const float x0 = float(hull[0].x), y0 = float(hull[0].y), x1 = float(hull[1].x), y1 = float(hull[1].y);
    cx = (x0 + x1) * 0.5f;
    cy = (y0 + y1) * 0.5f;
    const double dx = double(x1) - double(x0), dy = double(y1) - double(y0);
    w = float(std::sqrt(dx * dx + dy * dy));
    angle = float(std::atan2(dy, dx));
  } else if (n == 1) {
    cx = float(hull[0].x);
    cy = float(hull[0].y);
  }
  const float a180 = angle * 180.f;
  box5[0] = cx;
  box5[1] = cy;
  box5[2] = w;
  box5[3] = h;
  box5[4] = float(double(a180) / 3.1415926535897932384626433832795);
}

}  // namespace sfm

extern "C" {

void sfm_guidance_default_options(sfm_guidance_options* o) {
  if (!o) return;
  o->h_bins = 60;       // CScanGuidance.cpp:14-17
  o->s_bins = 50;
  o->threshold = 0.01;
  o->alpha = 0.9;
  o->ema = 0;           // _frameCount is never incremented: the histogram is replaced
  o->reserved = 0;
}

int sfm_min_area_rect(int32_t n, const int32_t* pts_xy, float* box5) {
  if (n < 0 || !box5 || (n && !pts_xy))
    return fail(SFM_EINVAL, "sfm_min_area_rect: NULL argument or negative size");
  std::vector<sfm::GPoint> p(static_cast<size_t>(n));
  for (int32_t i = 0; i < n; ++i) p[size_t(i)] = {pts_xy[2 * size_t(i)], pts_xy[2 * size_t(i) + 1]};
  sfm::guidance_min_area_rect(p, box5);
  return 0;
}

}  // extern "C"
