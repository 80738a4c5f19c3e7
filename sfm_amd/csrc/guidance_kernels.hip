// Scan guidance on the device (CScanGuidance::calculateMask, CScanGuidance.cpp:
// 39-105): the O(map points) and O(pixels) part of the call.
// The arithmetic is the restatement in tests/guidance_ref.py, bit for bit
// (compiled unfused); the hull of the thresholded pixels and cv::minAreaRect
// run on the host (guidance_host.cpp) on at most two points per row.
//
// Per call, on the handle's stream: one upload of the colour frame (through a
// pinned staging copy), one memset of the control block, four kernels,
//   k_guid_project  one lane per map point: centroid partial sums (fixed-order
//                   tree per workgroup), projection, pixel and quarter-pixel
//                   rounding, integer atomicMax into per-row left/right extents
//   k_guid_hull     one workgroup: the centroid sums, the hull of the <= 2 rows
//                   extent points as a per-row pixel interval, its area and
//                   its vertex count
//   k_guid_pixels   one lane per quarter-size pixel: resize taps from the
//                   frame, HSV, the packed bin pair, the masked histogram (LDS
//                   integer adds, flushed with integer global adds)
//   k_guid_backproject  one workgroup per row: the histogram state (replace
//                   or blend), the back-projection, the threshold and the
//                   row's extent of accepted pixels
// one download (48 bytes + 12 bytes per row) and ONE host synchronisation.
// Integer atomics only: two runs on equal input give equal bits.
//
// The map's points are read where they live (map_internal.h).  Every map call
// has completed by the time it returns; the guidance stream is still ordered
// after the map's stream with an event, which keeps that rule local.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "guidance_internal.h"
#include "map_internal.h"
#include "sfm_trace.h"
#include "dev_mem.h"

namespace sfm {
namespace {

int gfail(int code, const std::string& m) { return fail(code, "sfm_guidance: " + m); }

constexpr int kProjectBlock = 256;
constexpr int kHullBlock = 256;
constexpr int kPixelBlock = 512;
constexpr int kRowBlock = 256;
constexpr int kLdsHistBins = 8192;    // up to 32 KB of LDS histogram; above: global adds
constexpr uint16_t kOutside = 0xFFFF;  // packed bin pair of a pixel outside either range

// Head of the control block (zeroed every call, downloaded with the rows).
struct GuidHead {
  double sum[3];   // of the live points, fixed order
  double area;     // of the hull
  int32_t n_projected, n_hull;
  int32_t pad[2];
};
static_assert(sizeof(GuidHead) == 48, "GuidHead layout");

struct Pose {
  double r[9], t[3], fx, fy, cx, cy;
};

// (a) one lane per map point slot
__global__ __launch_bounds__(kProjectBlock) void k_guid_project(int n, const double* __restrict__ X,
                                                                const uint8_t* __restrict__ live, Pose p, int W,
                                                                int H, int ws, int hs, double* __restrict__ partial,
                                                                int32_t* __restrict__ ext, GuidHead* __restrict__ head) {
  __shared__ double sh[3][kProjectBlock];
  __shared__ int kept_sh;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kProjectBlock + tid;
  if (tid == 0) kept_sh = 0;
  double x0 = 0.0, x1 = 0.0, x2 = 0.0;
  const bool on = i < n && (!live || live[i]);
  if (on) {
    x0 = X[3 * size_t(i)];
    x1 = X[3 * size_t(i) + 1];
    x2 = X[3 * size_t(i) + 2];
  }
  sh[0][tid] = x0;
  sh[1][tid] = x1;
  sh[2][tid] = x2;
  __syncthreads();
  if (on) {
    const double c0 = p.r[0] * x0 + p.r[1] * x1 + p.r[2] * x2 + p.t[0];
    const double c1 = p.r[3] * x0 + p.r[4] * x1 + p.r[5] * x2 + p.t[1];
    const double c2 = p.r[6] * x0 + p.r[7] * x1 + p.r[8] * x2 + p.t[2];
    const double u = rint(c0 / c2 * p.fx + p.cx), v = rint(c1 / c2 * p.fy + p.cy);  // cvRound
    if (c2 > 0.0 && u >= 0.0 && u < double(W) && v >= 0.0 && v < double(H)) {
      // pts2dM *= 0.25 on an int matrix; at most ws + 1, hs + 1
      const int us = min(int(rint(u * 0.25)), ws + 1), vs = min(int(rint(v * 0.25)), hs + 1);
      atomicMax(&ext[2 * vs], ws + 2 - us);   // left extent, stored reversed (0 = empty row)
      atomicMax(&ext[2 * vs + 1], us + 1);    // right extent + 1
      atomicAdd(&kept_sh, 1);
    }
  }
  for (int s = kProjectBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      sh[0][tid] += sh[0][tid + s];
      sh[1][tid] += sh[1][tid + s];
      sh[2][tid] += sh[2][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    partial[3 * size_t(blockIdx.x)] = sh[0][0];
    partial[3 * size_t(blockIdx.x) + 1] = sh[1][0];
    partial[3 * size_t(blockIdx.x) + 2] = sh[2][0];
    if (kept_sh) atomicAdd(&head->n_projected, kept_sh);
  }
}

// a / b > c / d for b, d > 0
__device__ inline bool frac_gt(int a, int b, int c, int d) { return a * d > c * b; }

// (b) one workgroup.  Rows 0 .. nr-1 (nr = hs + 2) hold each row's leftmost and
// rightmost quarter-pixel; only those can be hull vertices.  The hull's left
// side is the lower convex envelope of xl over the rows, its right side the
// upper concave envelope of xr: row i is on the left envelope iff the steepest
// slope reaching it from above is <= the shallowest slope leaving it (exact
// cross-multiplied integers; < : a strict vertex).  A row's mask interval is
// the chord between the envelope rows around it, rounded inwards.
__global__ __launch_bounds__(kHullBlock) void k_guid_hull(int nr, int ws, int hs, int n_partial,
                                                          const double* __restrict__ partial,
                                                          const int32_t* __restrict__ ext, int32_t* __restrict__ rowiv,
                                                          GuidHead* __restrict__ head) {
  extern __shared__ int32_t lds[];
  int32_t* xl = lds;             // [nr]  -1: empty row
  int32_t* xr = lds + nr;        // [nr]
  int32_t* fl = lds + 2 * nr;    // [nr]  0: inside, 1: on the envelope, 2: strict vertex
  int32_t* fr = lds + 3 * nr;    // [nr]
  __shared__ double sh[3][kHullBlock];
  __shared__ int y_first, y_last, twice_area, n_strict;
  const int tid = threadIdx.x;
  if (tid == 0) {
    y_first = nr;
    y_last = -1;
    twice_area = 0;
    n_strict = 0;
  }
  // the centroid sums: lane-strided in order, then the fixed tree
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int b = tid; b < n_partial; b += kHullBlock) {
    s0 += partial[3 * size_t(b)];
    s1 += partial[3 * size_t(b) + 1];
    s2 += partial[3 * size_t(b) + 2];
  }
  sh[0][tid] = s0;
  sh[1][tid] = s1;
  sh[2][tid] = s2;
  __syncthreads();
  for (int y = tid; y < nr; y += kHullBlock) {
    const int a = ext[2 * y], b = ext[2 * y + 1];
    xl[y] = b ? ws + 2 - a : -1;
    xr[y] = b ? b - 1 : -1;
    if (b) {
      atomicMin(&y_first, y);
      atomicMax(&y_last, y);
    }
  }
  for (int s = kHullBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      sh[0][tid] += sh[0][tid + s];
      sh[1][tid] += sh[1][tid + s];
      sh[2][tid] += sh[2][tid + s];
    }
    __syncthreads();
  }
  const int y0 = y_first, y1 = y_last;
  for (int i = tid; i < nr; i += kHullBlock) {
    int l = 0, r = 0;
    if (xl[i] >= 0) {
      if (i == y0 || i == y1) {
        l = r = 2;
      } else {
        // steepest / shallowest slope (dx over dy) from the rows above and to the rows below
        int lmax_n = 0, lmax_d = 0, rmin_n = 0, rmin_d = 0;  // from above (d = 0: none yet)
        for (int a = y0; a < i; ++a) {
          if (xl[a] < 0) continue;
          const int d = i - a, nl = xl[i] - xl[a], nrr = xr[i] - xr[a];
          if (!lmax_d || frac_gt(nl, d, lmax_n, lmax_d)) lmax_n = nl, lmax_d = d;
          if (!rmin_d || frac_gt(rmin_n, rmin_d, nrr, d)) rmin_n = nrr, rmin_d = d;
        }
        int lmin_n = 0, lmin_d = 0, rmax_n = 0, rmax_d = 0;  // to below
        for (int b = i + 1; b <= y1; ++b) {
          if (xl[b] < 0) continue;
          const int d = b - i, nl = xl[b] - xl[i], nrr = xr[b] - xr[i];
          if (!lmin_d || frac_gt(lmin_n, lmin_d, nl, d)) lmin_n = nl, lmin_d = d;
          if (!rmax_d || frac_gt(nrr, d, rmax_n, rmax_d)) rmax_n = nrr, rmax_d = d;
        }
        // left: convex from below, on it iff lmax <= lmin; right: concave, rmin >= rmax
        l = frac_gt(lmax_n, lmax_d, lmin_n, lmin_d) ? 0 : (frac_gt(lmin_n, lmin_d, lmax_n, lmax_d) ? 2 : 1);
        r = frac_gt(rmax_n, rmax_d, rmin_n, rmin_d) ? 0 : (frac_gt(rmin_n, rmin_d, rmax_n, rmax_d) ? 2 : 1);
      }
    }
    fl[i] = l;
    fr[i] = r;
  }
  __syncthreads();
  for (int y = tid; y < nr; y += kHullBlock) {
    int lo = ws, hi = -1;
    if (y >= y0 && y <= y1) {
      int a = y, b = y;
      while (!fl[a]) --a;   // rows y0 and y1 are on both envelopes
      while (!fl[b]) ++b;
      lo = a == b ? xl[a] : (xl[a] * (b - a) + (xl[b] - xl[a]) * (y - a) + (b - a - 1)) / (b - a);  // ceil, >= 0
      if (fl[y] && y < y1) {  // the envelope edge leaving this row
        int c = y + 1;
        while (!fl[c]) ++c;
        atomicAdd(&twice_area, -(xl[y] + xl[c]) * (c - y));
      }
      a = y, b = y;
      while (!fr[a]) --a;
      while (!fr[b]) ++b;
      hi = a == b ? xr[a] : (xr[a] * (b - a) + (xr[b] - xr[a]) * (y - a)) / (b - a);  // floor, >= 0
      if (fr[y] && y < y1) {
        int c = y + 1;
        while (!fr[c]) ++c;
        atomicAdd(&twice_area, (xr[y] + xr[c]) * (c - y));
      }
      const int strict = (fl[y] == 2) + (fr[y] == 2) - ((y == y0 || y == y1) && xl[y] == xr[y]);
      if (strict) atomicAdd(&n_strict, strict);
      lo = max(lo, 0);
      hi = min(hi, ws - 1);
    }
    if (y < hs) {
      rowiv[2 * y] = lo;
      rowiv[2 * y + 1] = hi;
    }
  }
  __syncthreads();
  if (tid == 0) {
    head->sum[0] = sh[0][0];
    head->sum[1] = sh[1][0];
    head->sum[2] = sh[2][0];
    head->area = double(twice_area) * 0.5;
    head->n_hull = n_strict;
  }
}

// cv::resize's INTER_LINEAR taps of one output coordinate (OpenCV 3.0, 8-bit)
__device__ inline void resize_tap(int d, double scale, int n_src, int& s0, int& s1, int& c0, int& c1) {
  float f = float((double(d) + 0.5) * scale - 0.5);
  int s = int(floorf(f));
  f = f - float(s);
  if (s < 0) f = 0.f, s = 0;
  if (s >= n_src - 1) f = 0.f, s = n_src - 1;
  c1 = int(rintf(f * 2048.f));
  c0 = int(rintf((1.f - f) * 2048.f));
  s0 = s;
  s1 = min(s + 1, n_src - 1);
}

// calcHist's uniform bin: cvFloor(double(value) * a + b); -1 = outside
__device__ inline int hist_bin(float v, int bins, double lo, double hi) {
  const double a = double(bins) / (hi - lo), b = -(a * lo);
  const double idx = floor(double(v) * a + b);
  return idx >= 0.0 && idx < double(bins) ? int(idx) : -1;
}

// (c) one lane per quarter-size pixel
__global__ __launch_bounds__(kPixelBlock) void k_guid_pixels(const uint8_t* __restrict__ img, int W, int H, int ws,
                                                             int hs, double scale_x, double scale_y, int h_bins,
                                                             int s_bins, int lds_hist,
                                                             const int32_t* __restrict__ rowiv,
                                                             uint16_t* __restrict__ bins, uint8_t* __restrict__ mask,
                                                             int32_t* __restrict__ cnt) {
  extern __shared__ int32_t hist[];
  const int nb = h_bins * s_bins;
  if (lds_hist) {
    for (int b = threadIdx.x; b < nb; b += kPixelBlock) hist[b] = 0;
    __syncthreads();
  }
  const int p = blockIdx.x * kPixelBlock + threadIdx.x;
  if (p < ws * hs) {
    const int dx = p % ws, dy = p / ws;
    int x0, x1, a0, a1, y0, y1, b0, b1;
    resize_tap(dx, scale_x, W, x0, x1, a0, a1);
    resize_tap(dy, scale_y, H, y0, y1, b0, b1);
    const uint8_t* r0 = img + size_t(y0) * 3 * W;
    const uint8_t* r1 = img + size_t(y1) * 3 * W;
    float f[3];
    for (int c = 0; c < 3; ++c) {
      const int S0 = int(r0[3 * x0 + c]) * a0 + int(r0[3 * x1 + c]) * a1;
      const int S1 = int(r1[3 * x0 + c]) * a0 + int(r1[3 * x1 + c]) * a1;
      const int o = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
      f[c] = float(min(max(o, 0), 255)) * float(1.0 / 255.0);
    }
    // cvtColor(.., CV_BGR2HSV), float
    const float b = f[0], g = f[1], r = f[2];
    float v = r, vmin = r;
    if (v < g) v = g;
    if (v < b) v = b;
    if (vmin > g) vmin = g;
    if (vmin > b) vmin = b;
    float diff = v - vmin;
    const float s = diff / float(double(fabsf(v)) + double(FLT_EPSILON));
    diff = float(60. / double(diff + FLT_EPSILON));
    float h;
    if (v == r)
      h = (g - b) * diff;
    else if (v == g)
      h = (b - r) * diff + 120.f;
    else
      h = (r - g) * diff + 240.f;
    if (h < 0.f) h += 360.f;
    const int hb = hist_bin(h, h_bins, 0.0, 360.0), sb = hist_bin(s, s_bins, 0.0, 1.0);
    const bool in = hb >= 0 && sb >= 0;
    const bool m = dx >= rowiv[2 * dy] && dx <= rowiv[2 * dy + 1];
    bins[p] = in ? uint16_t(hb * s_bins + sb) : kOutside;
    mask[p] = m ? 1 : 0;
    if (in && m) atomicAdd(lds_hist ? &hist[hb * s_bins + sb] : &cnt[hb * s_bins + sb], 1);
  }
  if (lds_hist) {
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += kPixelBlock)
      if (hist[b]) atomicAdd(&cnt[b], hist[b]);
  }
}

// (d) one workgroup per quarter-size row
__global__ __launch_bounds__(kRowBlock) void k_guid_backproject(int ws, int nb, const uint16_t* __restrict__ bins,
                                                                const int32_t* __restrict__ cnt,
                                                                const float* __restrict__ old_state,
                                                                float* __restrict__ new_state, int blend, float af,
                                                                float bf, double threshold,
                                                                const GuidHead* __restrict__ head,
                                                                float* __restrict__ bproj, int32_t* __restrict__ acc) {
  __shared__ int lo, hi, count;
  const int y = blockIdx.x;
  if (threadIdx.x == 0) {
    lo = ws;
    hi = -1;
    count = 0;
  }
  __syncthreads();
  // _hist = hist, or alpha * hist + (1 - alpha) * _hist in float
  auto state = [&](int b) {
    const float c = float(cnt[b]);
    return blend ? c * af + old_state[b] * bf : c;
  };
  for (int b = blockIdx.x * kRowBlock + threadIdx.x; b < nb; b += gridDim.x * kRowBlock) new_state[b] = state(b);
  const double area = head->area;
  for (int x = threadIdx.x; x < ws; x += kRowBlock) {
    const uint16_t b = bins[size_t(y) * ws + x];
    const float bp = b == kOutside ? 0.f : state(b);
    bproj[size_t(y) * ws + x] = bp;
    if (double(bp) / area > threshold) {   // x / 0 = inf is accepted, 0 / 0 is not
      atomicMin(&lo, x);
      atomicMax(&hi, x);
      atomicAdd(&count, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc[3 * y] = lo;
    acc[3 * y + 1] = hi;
    acc[3 * y + 2] = count;
  }
}

bool finite_n(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace
}  // namespace sfm

using namespace sfm;

// The stream first: members are destroyed in reverse order, so it goes last.
struct sfm_guidance {
  Stream s;
  int device = 0, W = 0, H = 0, ws = 0, hs = 0, nb = 0;
  sfm_guidance_options opt{};
  Event ev_map, ev[4];
  DevArr<uint8_t> d_img;         // [H][3 W]
  PinArr<uint8_t> h_img;         // pinned staging copy of the frame
  DevArr<uint8_t> d_ctl;         // GuidHead | acc [hs][3] | ext [hs+2][2] | cnt [nb]   (zeroed every call)
  PinArr<uint8_t> h_ctl;         // pinned: GuidHead | acc
  DevArr<int32_t> d_rowiv;       // [hs][2] mask interval of each row
  DevArr<uint16_t> d_bins;       // [hs][ws]
  DevArr<uint8_t> d_mask;        // [hs][ws]
  DevArr<float> d_bproj;         // [hs][ws]
  DevArr<float> d_state[2];      // the histogram state, double-buffered
  int cur = 0;                   // d_state[cur] is _hist
  bool have_state = false;
  DevArr<double> d_pts;          // sfm_guidance_update_points' upload
  DevArr<double> d_partial;      // [blocks][3]
  std::vector<int32_t> extents;  // [hs][2] of the last update
  bool updated = false;
  float ms[3] = {0.f, 0.f, 0.f};

  size_t head_bytes() const { return sizeof(GuidHead) + sizeof(int32_t) * 3 * size_t(hs); }
  size_t ctl_bytes() const { return head_bytes() + sizeof(int32_t) * (2 * size_t(hs + 2) + size_t(nb)); }
  GuidHead* head() const { return d_ctl.as<GuidHead>(); }
  int32_t* acc() const { return reinterpret_cast<int32_t*>(d_ctl + sizeof(GuidHead)); }
  int32_t* ext() const { return acc() + 3 * size_t(hs); }
  int32_t* cnt() const { return ext() + 2 * size_t(hs + 2); }
};

namespace {

// Room for `need` doubles (contents dropped when it grows).
int reserve(DevArr<double>& b, int64_t need, hipStream_t s) {
  const int64_t cap = int64_t(b.bytes() / sizeof(double));
  const int64_t want = std::max<int64_t>({need, 2 * cap, 1024});
  if (b.reserve(size_t(need) * sizeof(double), size_t(want) * sizeof(double), s))
    return gfail(SFM_ENOMEM, "hipMalloc failed (points)");
  return 0;
}

int check_args(const sfm_guidance* h, const uint8_t* img, int32_t stride, const double* R9, const double* t3,
               const double* K9, const sfm_guidance_result* out) {
  if (!h || !img || !R9 || !t3 || !K9 || !out) return gfail(SFM_EINVAL, "NULL argument");
  if (int64_t(stride) < 3 * int64_t(h->W)) return gfail(SFM_EINVAL, "stride < 3 * width");
  if (!finite_n(R9, 9) || !finite_n(t3, 3) || !finite_n(K9, 9)) return gfail(SFM_EINVAL, "K, R or t is not finite");
  return 0;
}

// Everything after the argument checks; X / live are device pointers.
int run(sfm_guidance* h, const double* X, const uint8_t* live, int n_slots, int n_live, const uint8_t* img,
        int32_t stride, const double* R9, const double* t3, const double* K9, sfm_guidance_result* out) {
  const int W = h->W, H = h->H, ws = h->ws, hs = h->hs;
  const int n_blocks = (n_slots + kProjectBlock - 1) / kProjectBlock;
  if (int rc = reserve(h->d_partial, 3 * int64_t(std::max(n_blocks, 1)), h->s)) return rc;
  for (int y = 0; y < H; ++y) std::memcpy(h->h_img + size_t(y) * 3 * W, img + size_t(y) * stride, 3 * size_t(W));
  bool ok = hipEventRecord(h->ev[0], h->s) == hipSuccess;
  ok = ok && hipMemcpyAsync(h->d_img, h->h_img, size_t(H) * 3 * W, hipMemcpyHostToDevice, h->s) == hipSuccess;
  ok = ok && hipEventRecord(h->ev[1], h->s) == hipSuccess;
  ok = ok && hipMemsetAsync(h->d_ctl, 0, h->ctl_bytes(), h->s) == hipSuccess;
  if (!ok) {
    (void)hipStreamSynchronize(h->s);  // nothing of this call stays queued on the staging copy
    return gfail(SFM_EIO, "upload failed");
  }
  Pose p;
  for (int i = 0; i < 9; ++i) p.r[i] = R9[i];
  for (int i = 0; i < 3; ++i) p.t[i] = t3[i];
  p.fx = K9[0];
  p.fy = K9[4];
  p.cx = K9[2];
  p.cy = K9[5];
  if (n_blocks)
    k_guid_project<<<n_blocks, kProjectBlock, 0, h->s>>>(n_slots, X, live, p, W, H, ws, hs, h->d_partial, h->ext(),
                                                         h->head());
  const int nr = hs + 2;
  k_guid_hull<<<1, kHullBlock, sizeof(int32_t) * 4 * size_t(nr), h->s>>>(nr, ws, hs, n_blocks, h->d_partial, h->ext(),
                                                                        h->d_rowiv, h->head());
  const int lds_hist = h->nb <= kLdsHistBins;
  k_guid_pixels<<<(ws * hs + kPixelBlock - 1) / kPixelBlock, kPixelBlock, lds_hist ? sizeof(int32_t) * size_t(h->nb) : 0,
                  h->s>>>(h->d_img, W, H, ws, hs, double(W) / double(ws), double(H) / double(hs), h->opt.h_bins,
                          h->opt.s_bins, lds_hist, h->d_rowiv, h->d_bins, h->d_mask, h->cnt());
  const int blend = h->opt.ema && h->have_state;
  k_guid_backproject<<<hs, kRowBlock, 0, h->s>>>(ws, h->nb, h->d_bins, h->cnt(), h->d_state[h->cur],
                                                 h->d_state[1 - h->cur], blend, float(h->opt.alpha),
                                                 float(1.0 - h->opt.alpha), h->opt.threshold, h->head(), h->d_bproj,
                                                 h->acc());
  ok = hipGetLastError() == hipSuccess && hipEventRecord(h->ev[2], h->s) == hipSuccess;
  ok = ok && hipMemcpyAsync(h->h_ctl, h->d_ctl, h->head_bytes(), hipMemcpyDeviceToHost, h->s) == hipSuccess;
  ok = ok && hipEventRecord(h->ev[3], h->s) == hipSuccess;
  if (hipStreamSynchronize(h->s) != hipSuccess || !ok) return gfail(SFM_EIO, "kernel or copy failed");
  h->cur = 1 - h->cur;
  h->have_state = true;
  h->updated = true;
  for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&h->ms[i], h->ev[i], h->ev[i + 1]);

  GuidHead head;
  std::memcpy(&head, h->h_ctl, sizeof head);
  const int32_t* acc = reinterpret_cast<const int32_t*>(h->h_ctl + sizeof(GuidHead));
  std::vector<GPoint> pts;
  pts.reserve(2 * size_t(hs));
  int32_t n_acc = 0;
  for (int y = 0; y < hs; ++y) {
    h->extents[2 * size_t(y)] = acc[3 * y];
    h->extents[2 * size_t(y) + 1] = acc[3 * y + 1];
    n_acc += acc[3 * y + 2];
    if (acc[3 * y + 1] >= 0) {
      pts.push_back({acc[3 * y], y});
      pts.push_back({acc[3 * y + 1], y});
    }
  }
  // the hull of the rows' extent points is the hull of every accepted pixel
  float box[5];
  guidance_min_area_rect(pts, box);
  const double inv_n = 1.0 / double(n_live);   // updateCentroid; NaN for an empty map
  for (int i = 0; i < 3; ++i) out->centroid[i] = head.sum[i] * inv_n;
  // _bbox.size, _bbox.center *= 1.0 / _scale
  const double up = 1.0 / 0.25;
  out->box_center[0] = float(double(box[0]) * up);
  out->box_center[1] = float(double(box[1]) * up);
  out->box_size[0] = float(double(box[2]) * up);
  out->box_size[1] = float(double(box[3]) * up);
  out->box_angle = box[4];
  out->n_points = n_live;
  out->n_projected = head.n_projected;
  out->n_hull = head.n_hull;
  out->n_accepted = n_acc;
  out->area = head.area;
  return 0;
}

}  // namespace

extern "C" {

int sfm_guidance_create(int32_t device, int32_t width, int32_t height, const sfm_guidance_options* options,
                        sfm_guidance** out) {
  if (!out) return gfail(SFM_EINVAL, "out is NULL");
  *out = nullptr;
  sfm_guidance_options o;
  sfm_guidance_default_options(&o);
  if (options) o = *options;
  if (width < 8 || height < 8 || width > 8192 || height > 8192)
    return gfail(SFM_EINVAL, "width and height must be in 8..8192");
  if (o.h_bins < 1 || o.h_bins > 256 || o.s_bins < 1 || o.s_bins > 256 || o.h_bins * o.s_bins > 65535)
    return gfail(SFM_EINVAL, "bin counts must be in 1..256 (and not both 256)");
  if (!std::isfinite(o.threshold) || !std::isfinite(o.alpha)) return gfail(SFM_EINVAL, "threshold or alpha is not finite");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return gfail(SFM_ENODEV, "no such device");
  if (hipSetDevice(device) != hipSuccess) return gfail(SFM_ENODEV, "hipSetDevice failed");
  auto* h = new sfm_guidance;
  h->device = device;
  h->W = width;
  h->H = height;
  h->ws = int(width * 0.25);   // Size(frame.cols * _scale, frame.rows * _scale)
  h->hs = int(height * 0.25);
  h->nb = o.h_bins * o.s_bins;
  h->opt = o;
  h->extents.assign(2 * size_t(h->hs), 0);
  const size_t px = size_t(h->ws) * h->hs;
  auto fixed = [](auto& buf, size_t bytes) { return buf.reserve(bytes, bytes, nullptr) == 0; };
  bool ok = h->s.create(hipStreamNonBlocking) == hipSuccess;
  ok = ok && h->ev_map.create(hipEventDisableTiming) == hipSuccess;
  for (auto& e : h->ev) ok = ok && e.create(hipEventDefault) == hipSuccess;
  ok = ok && fixed(h->d_img, size_t(height) * 3 * width) && fixed(h->h_img, size_t(height) * 3 * width);
  ok = ok && fixed(h->d_ctl, h->ctl_bytes()) && fixed(h->h_ctl, h->head_bytes());
  ok = ok && fixed(h->d_rowiv, sizeof(int32_t) * 2 * size_t(h->hs)) && fixed(h->d_bins, sizeof(uint16_t) * px);
  ok = ok && fixed(h->d_mask, px) && fixed(h->d_bproj, sizeof(float) * px);
  for (auto& st : h->d_state) {
    ok = ok && fixed(st, sizeof(float) * size_t(h->nb));
    ok = ok && hipMemset(st, 0, sizeof(float) * size_t(h->nb)) == hipSuccess;
  }
  if (!ok) {
    sfm_guidance_destroy(h);
    return gfail(SFM_ENOMEM, "stream, event or buffer creation failed");
  }
  *out = h;
  return 0;
}

int sfm_guidance_destroy(sfm_guidance* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->s) (void)hipStreamSynchronize(h->s);
  delete h;
  return 0;
}

int sfm_guidance_update(sfm_guidance* h, sfm_map* map, const uint8_t* img, int32_t stride, const double* R9,
                        const double* t3, const double* K9, sfm_guidance_result* out) {
  SFM_TRACE("sfm_guidance_update");
  if (!map) return gfail(SFM_EINVAL, "NULL argument");
  if (int rc = check_args(h, img, stride, R9, t3, K9, out)) return rc;
  const MapPointsView v = map_points_view(map);
  if (v.device != h->device) return gfail(SFM_EINVAL, "the map and the handle are on different devices");
  if (hipSetDevice(h->device) != hipSuccess) return gfail(SFM_ENODEV, "hipSetDevice failed");
  if (hipEventRecord(h->ev_map, v.stream) != hipSuccess || hipStreamWaitEvent(h->s, h->ev_map, 0) != hipSuccess)
    return gfail(SFM_EIO, "ordering after the map's stream failed");
  return run(h, v.X, v.live, v.n_slots, v.n_live, img, stride, R9, t3, K9, out);
}

int sfm_guidance_update_points(sfm_guidance* h, int32_t n, const double* pts3d, const uint8_t* img, int32_t stride,
                               const double* R9, const double* t3, const double* K9, sfm_guidance_result* out) {
  SFM_TRACE("sfm_guidance_update_points");
  if (int rc = check_args(h, img, stride, R9, t3, K9, out)) return rc;
  if (n < 0 || (n && !pts3d)) return gfail(SFM_EINVAL, n < 0 ? "negative size" : "NULL argument");
  if (hipSetDevice(h->device) != hipSuccess) return gfail(SFM_ENODEV, "hipSetDevice failed");
  if (int rc = reserve(h->d_pts, 3 * int64_t(n), h->s)) return rc;
  if (n && hipMemcpyAsync(h->d_pts, pts3d, sizeof(double) * 3 * size_t(n), hipMemcpyHostToDevice, h->s) != hipSuccess)
    return gfail(SFM_EIO, "upload failed (points)");
  return run(h, h->d_pts, nullptr, n, n, img, stride, R9, t3, K9, out);
}

int sfm_guidance_read_planes(sfm_guidance* h, uint8_t* mask, int16_t* bins, float* hist, float* bproj,
                             int32_t* extents) {
  if (!h) return gfail(SFM_EINVAL, "NULL handle");
  if (!h->updated) return gfail(SFM_EINVAL, "no update yet");
  if (hipSetDevice(h->device) != hipSuccess) return gfail(SFM_ENODEV, "hipSetDevice failed");
  const size_t px = size_t(h->ws) * h->hs;
  bool ok = true;
  if (mask) ok = ok && hipMemcpy(mask, h->d_mask, px, hipMemcpyDeviceToHost) == hipSuccess;
  if (bins) {
    std::vector<uint16_t> b(px);
    ok = ok && hipMemcpy(b.data(), h->d_bins, sizeof(uint16_t) * px, hipMemcpyDeviceToHost) == hipSuccess;
    for (size_t i = 0; ok && i < px; ++i) {
      const bool outside = b[i] == kOutside;
      bins[2 * i] = outside ? int16_t(-1) : int16_t(b[i] / h->opt.s_bins);
      bins[2 * i + 1] = outside ? int16_t(-1) : int16_t(b[i] % h->opt.s_bins);
    }
  }
  if (hist)
    ok = ok && hipMemcpy(hist, h->d_state[h->cur], sizeof(float) * size_t(h->nb), hipMemcpyDeviceToHost) == hipSuccess;
  if (bproj) ok = ok && hipMemcpy(bproj, h->d_bproj, sizeof(float) * px, hipMemcpyDeviceToHost) == hipSuccess;
  if (extents) std::memcpy(extents, h->extents.data(), sizeof(int32_t) * h->extents.size());
  return ok ? 0 : gfail(SFM_EIO, "download failed");
}

int sfm_guidance_last_time(sfm_guidance* h, double* ms3) {
  if (!h || !ms3) return gfail(SFM_EINVAL, "NULL argument");
  for (int i = 0; i < 3; ++i) ms3[i] = double(h->ms[i]);
  return 0;
}

}  // extern "C"
