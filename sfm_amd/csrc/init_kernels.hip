// Two-view map initialisation: steps 2-5 of CSfM::init
// (/root/reference/CSfM.cpp:842-946) on gfx950, behind sfm_two_view_init.
// OpenCV 3.0 and GeometryUtils are absent; the semantics are restated once in
// tests/two_view_ref.py (parity with OpenCV / GeometryUtils unpinned) and
// this file computes the same:
//   * findFundamentalMat(FM_RANSAC): RANSAC over 7-point subsets drawn by
//     cv::RNG(uint64(-1)), run7Point on raw pixels (null space of the 7x9
//     system by cv::SVD, the cubic in lambda, up to three models per subset
//     tested in order), error = max of the two squared point-line distances
//     stored as float, inlier when err <= float(thr^2), a model accepted when
//     its count beats max(best, 6), the bound shrunk by RANSACUpdateNumIters,
//     no refit;
//   * findHomography(method 0): normalised DLT over all matches, then
//     cv::LMSolver (10 iterations) on the forward transfer error;
//   * both rounded to float32; the scores of CSfM.cpp:415-469, the average
//     errors, the decompositions, the cheirality vote, the triangulation and
//     the final filter in fp64 on the rounded matrices.
//
// Device mapping (the stage is latency bound: n is a few hundred to a few
// thousand; six launches on one stream, no host round trip in between):
//   k_tv_subsets  one thread draws every subset of the bound (sequential RNG)
//   k_tv_seven    one lane per subset: the 7-point solve
//   k_tv_count    one workgroup per (subset, root): inlier count, fixed order
//   k_tv_model    one workgroup: the replay of the sequential acceptance rule
//                 (the bound only shrinks, so evaluating the whole bound and
//                 replaying gives the sequential result), the mask, the DLT and
//                 LM normal equations, scores and errors as fixed-order block
//                 reductions, the 3x3 SVDs and the candidates
//   k_tv_vote     one workgroup per candidate: the cheirality vote
//   k_tv_final    one workgroup: the winner, triangulation and final filter
// Every sum is a fixed-order reduction (lane butterfly, then the waves in
// order): results are bitwise reproducible; no floating-point atomics.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include "sfm_trace.h"
#include "../../include/sfm_amd.h"
#include "cv_linalg.h"
#include "tri_point.h"
#include "dev_mem.h"


namespace sfm {
namespace {

constexpr int kSub = 7;          // RANSAC subset size
constexpr int kTvMaxIters = 2048;
constexpr int kMinPoints = 15;   // below it OpenCV switches to LMedS (not restated)
constexpr int kBlock = 256;      // the single-workgroup kernels
constexpr int kWaves = kBlock / 64;
constexpr int kMaxCand = 8;

// result head (doubles), followed by X [n][3], then f_mask [n], keep [n] bytes
enum : int {
  hModel = 0, hKept = 1, hH = 2, hF = 11, hScores = 20, hAvgErr = 22, hR = 23, hT = 32, hBranch = 35, hNCand = 36,
  hBest = 37, hHead = 40
};

struct TvArgs {
  double K0[9], K1[9];
  sfm_two_view_options o;
  double cos_par;  // cos(min_parallax_deg)
  float thr32;     // float(f_ransac_threshold^2)
  int n, iters;
};

__device__ __forceinline__ double det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
__device__ void inv3(const double* M, double* o) {
  double c[9] = {M[4] * M[8] - M[5] * M[7], M[2] * M[7] - M[1] * M[8], M[1] * M[5] - M[2] * M[4],
                 M[5] * M[6] - M[3] * M[8], M[0] * M[8] - M[2] * M[6], M[2] * M[3] - M[0] * M[5],
                 M[3] * M[7] - M[4] * M[6], M[1] * M[6] - M[0] * M[7], M[0] * M[4] - M[1] * M[3]};
  const double det = M[0] * c[0] + M[1] * c[3] + M[2] * c[6];
  const double id = 1.0 / det;
  for (int i = 0; i < 9; ++i) o[i] = c[i] * id;
}
__device__ void mul3(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// cv::solveCubic (3.0): a0 x^3 + a1 x^2 + a2 x + a3 -> the number of real roots
__device__ int solve_cubic(double a0, double a1, double a2, double a3, double r[3]) {
  if (a0 == 0) {
    if (a1 == 0) {
      if (a2 == 0) return 0;
      r[0] = -a3 / a2;
      return 1;
    }
    double d = a2 * a2 - 4 * a1 * a3;
    if (d < 0) return 0;
    d = sqrt(d);
    const double q1 = (-a2 + d) * 0.5, q2 = (a2 + d) * -0.5;
    if (fabs(q1) > fabs(q2)) { r[0] = q1 / a1; r[1] = a3 / q1; }
    else { r[0] = q2 / a1; r[1] = a3 / q2; }
    return d > 0 ? 2 : 1;
  }
  a0 = 1.0 / a0;
  a1 *= a0; a2 *= a0; a3 *= a0;
  const double Q = (a1 * a1 - 3 * a2) * (1.0 / 9);
  const double R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1.0 / 54);
  const double Qc = Q * Q * Q;
  double d = Qc - R * R;
  if (d >= 0) {
    const double theta = Qc > 0 ? acos(fmin(1.0, fmax(-1.0, R / sqrt(Qc)))) : 0.0;
    const double t0 = -2 * sqrt(Q), t1 = theta * (1.0 / 3), t2 = a1 * (1.0 / 3);
    r[0] = t0 * cos(t1) - t2;
    r[1] = t0 * cos(t1 + 2.0 * M_PI / 3) - t2;
    r[2] = t0 * cos(t1 + 4.0 * M_PI / 3) - t2;
    return 3;
  }
  d = sqrt(-d);
  double e = pow(d + fabs(R), 1.0 / 3);
  if (R > 0) e = -e;
  r[0] = (e + Q / e) - a1 * (1.0 / 3);
  return 1;
}

// cv::RNG(uint64(-1)) subsets of the whole bound (getSubset: 7 distinct draws)
__global__ void k_tv_subsets(int n, int iters, int* __restrict__ sub) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint64_t state = ~0ull;
  for (int it = 0; it < iters; ++it) {
    int idx[kSub];
    for (int i = 0; i < kSub; ++i) {
      int v;
      while (true) {
        v = int(cv_rng_next(state) % unsigned(n));
        int j = 0;
        for (; j < i; ++j)
          if (idx[j] == v) break;
        if (j == i) break;
      }
      idx[i] = v;
    }
    for (int i = 0; i < kSub; ++i) sub[it * kSub + i] = idx[i];
  }
}

// run7Point of one subset per lane: models [iters][3][9], nm [iters].  The
// null space of the 7x9 system as cv::SVD(FULL_UV) yields it: the SVD of the
// transpose (one-sided Jacobi on the 7 rows of the system), then the two
// missing right singular vectors completed from cv::RNG(0x12345678) vectors
// orthogonalised twice against the rows before them (JacobiSVDImpl_).
__global__ __launch_bounds__(64) void k_tv_seven(int iters, const float* __restrict__ p0,
                                                 const float* __restrict__ p1, const int* __restrict__ sub,
                                                 double* __restrict__ models, int* __restrict__ nm) {
  const int it = blockIdx.x * 64 + threadIdx.x;
  if (it >= iters) return;
  double U[9][9], w[kSub], Vt[kSub][kSub];  // rows 0..6 of U: the system's rows, then its right singular vectors
#pragma unroll
  for (int i = 0; i < kSub; ++i) {
    const int q = sub[it * kSub + i];
    const double x0 = p0[2 * q], y0 = p0[2 * q + 1], x1 = p1[2 * q], y1 = p1[2 * q + 1];
    U[i][0] = x1 * x0; U[i][1] = x1 * y0; U[i][2] = x1;
    U[i][3] = y1 * x0; U[i][4] = y1 * y0; U[i][5] = y1;
    U[i][6] = x0; U[i][7] = y0; U[i][8] = 1.0;
  }
  cv_svd_at<9, kSub, false>(reinterpret_cast<double (&)[kSub][9]>(U), w, Vt);
  {
    uint64_t rng = 0x12345678ull;
    const double eps = DBL_EPSILON * 10;
#pragma unroll
    for (int i = kSub; i < 9; ++i) {
      double sd = 0.0;
      for (int ii = 0; ii < 100 && sd <= DBL_MIN; ++ii) {
        const double val0 = 1.0 / 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) U[i][k] = (cv_rng_next(rng) & 256) != 0 ? val0 : -val0;
        for (int it2 = 0; it2 < 2; ++it2)
#pragma unroll
          for (int j = 0; j < i; ++j) {
            sd = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) sd += U[i][k] * U[j][k];
            double asum = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
              const double t = U[i][k] - sd * U[j][k];
              U[i][k] = t;
              asum += fabs(t);
            }
            asum = asum > eps * 100 ? 1.0 / asum : 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) U[i][k] *= asum;
          }
        sd = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) sd += U[i][k] * U[i][k];
        sd = sqrt(sd);
      }
      const double sc = sd > DBL_MIN ? 1.0 / sd : 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) U[i][k] *= sc;
    }
  }
  double f1[9], f2[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    f2[i] = U[8][i];
    f1[i] = U[7][i] - f2[i];  // f = lambda (f1 - f2) + f2
  }
  // det(lambda A + B) = det A l^3 + c1 l^2 + c2 l + det B; c2 (c1) = the sum
  // over rows of det B (A) with that row taken from A (B)
  double c1 = 0.0, c2 = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double M[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = k / 3 == i ? f1[k] : f2[k];
    c2 += det3(M);
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = k / 3 == i ? f2[k] : f1[k];
    c1 += det3(M);
  }
  double r[3] = {0.0, 0.0, 0.0};
  const int nr = solve_cubic(det3(f1), c1, c2, det3(f2), r);
  nm[it] = nr;
  for (int k = 0; k < nr; ++k) {
    double lam = r[k], mu = 1.0, f8 = 0.0;
    const double s = f1[8] * r[k] + f2[8];
    if (fabs(s) > DBL_EPSILON) {
      mu = 1.0 / s;
      lam *= mu;
      f8 = 1.0;
    }
    double* o = models + (size_t(it) * 3 + k) * 9;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = f1[i] * lam + f2[i] * mu;
    o[8] = f8;
  }
}

// The residual x1^T F x0 against the line F x0 in image 1 (d1, squared norm
// n1) and against F^T x1 in image 0 (d0, n0).
struct LineTerms {
  double d1, n1, d0, n0;
};
__device__ __forceinline__ LineTerms line_terms(const double* F, double x0, double y0, double x1, double y1) {
  LineTerms t;
  double a = F[0] * x0 + F[1] * y0 + F[2];
  double b = F[3] * x0 + F[4] * y0 + F[5];
  double c = F[6] * x0 + F[7] * y0 + F[8];
  t.n1 = a * a + b * b;
  t.d1 = x1 * a + y1 * b + c;
  a = F[0] * x1 + F[3] * y1 + F[6];
  b = F[1] * x1 + F[4] * y1 + F[7];
  c = F[2] * x1 + F[5] * y1 + F[8];
  t.n0 = a * a + b * b;
  t.d0 = x0 * a + y0 * b + c;
  return t;
}
// FMEstimatorCallback::computeError + findInliers
__device__ __forceinline__ bool f_inlier(const double* F, const float* __restrict__ p0, const float* __restrict__ p1,
                                         int q, float thr) {
  const LineTerms t = line_terms(F, p0[2 * q], p0[2 * q + 1], p1[2 * q], p1[2 * q + 1]);
  const double e0 = t.d0 * t.d0 * (1.0 / t.n0), e1 = t.d1 * t.d1 * (1.0 / t.n1);
  const double e = (e0 > e1 || e0 != e0) ? e0 : e1;  // NaN propagates
  return float(e) <= thr;
}

__global__ __launch_bounds__(256) void k_tv_count(int n, const float* __restrict__ p0, const float* __restrict__ p1,
                                                  const double* __restrict__ models, const int* __restrict__ nm,
                                                  float thr, int* __restrict__ cnt) {
  __shared__ int sh[4];
  const int m = blockIdx.x;  // (subset, root)
  if (m % 3 >= nm[m / 3]) {
    if (threadIdx.x == 0) cnt[m] = 0;
    return;
  }
  double F[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = models[size_t(m) * 9 + i];
  int c = 0;
  for (int q = threadIdx.x; q < n; q += 256) c += f_inlier(F, p0, p1, q, thr) ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[m] = sh[0] + sh[1] + sh[2] + sh[3];
}

// Fixed-order block sums: the lane butterfly (every lane ends with the same
// value), then the waves in order.  sh: kWaves * NV doubles.
template <int NV>
__device__ void block_sum(double (&v)[NV], double* sh) {
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
  __syncthreads();  // (earlier readers of sh done)
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) sh[(threadIdx.x >> 6) * NV + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += sh[w * NV + k];
    v[k] = s;
  }
}
__device__ double block_max(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s = fmax(s, sh[w]);
  return s;
}

// x = A^-1 b for the 8x8 normal equations (partial pivoting); false: singular
__device__ bool solve8(const double* A, const double* b, double* x) {
  double M[8][9];
  for (int i = 0; i < 8; ++i) {
    for (int j = 0; j < 8; ++j) M[i][j] = A[8 * i + j];
    M[i][8] = b[i];
  }
  for (int k = 0; k < 8; ++k) {
    int p = k;
    for (int i = k + 1; i < 8; ++i)
      if (fabs(M[i][k]) > fabs(M[p][k])) p = i;
    if (M[p][k] == 0.0) return false;
    if (p != k)
      for (int j = k; j < 9; ++j) { const double t = M[k][j]; M[k][j] = M[p][j]; M[p][j] = t; }
    for (int i = k + 1; i < 8; ++i) {
      const double f = M[i][k] / M[k][k];
      for (int j = k; j < 9; ++j) M[i][j] -= f * M[k][j];
    }
  }
  for (int i = 7; i >= 0; --i) {
    double s = M[i][8];
    for (int j = i + 1; j < 8; ++j) s -= M[i][j] * x[j];
    x[i] = s / M[i][i];
  }
  return true;
}

// HomographyRefineCallback::compute over this thread's matches: acc = the
// upper triangle of J^T J (36) | J^T r (8) | |r|^2 (kJ), or |r|^2 alone;
// returns the thread's max |r|.
template <bool kJ>
__device__ double h_accumulate(int n, const float* __restrict__ p0, const float* __restrict__ p1, const double* h,
                               double (&acc)[kJ ? 45 : 1]) {
  double rmax = 0.0;
#pragma unroll
  for (int k = 0; k < (kJ ? 45 : 1); ++k) acc[k] = 0.0;
  for (int q = threadIdx.x; q < n; q += kBlock) {
    const double Mx = p0[2 * q], My = p0[2 * q + 1];
    double ww = h[6] * Mx + h[7] * My + 1.0;
    ww = fabs(ww) > DBL_EPSILON ? 1.0 / ww : 0.0;
    const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww, yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
    const double rx = xi - double(p1[2 * q]), ry = yi - double(p1[2 * q + 1]);
    rmax = fmax(rmax, fmax(fabs(rx), fabs(ry)));
    if constexpr (kJ) {
      const double Jx[8] = {Mx * ww, My * ww, ww, 0.0, 0.0, 0.0, -Mx * ww * xi, -My * ww * xi};
      const double Jy[8] = {0.0, 0.0, 0.0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
      int k = 0;
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = a; b < 8; ++b, ++k) acc[k] += Jx[a] * Jx[b] + Jy[a] * Jy[b];
#pragma unroll
      for (int a = 0; a < 8; ++a) acc[36 + a] += Jx[a] * rx + Jy[a] * ry;
      acc[44] += rx * rx + ry * ry;
    } else {
      acc[0] += rx * rx + ry * ry;
    }
  }
  return rmax;
}

// cv::LMSolver's state (thread 0 writes, every thread reads after a barrier)
struct LmState {
  double x[8], xd[8], A[64], v[8], D[8], d[8];
  double S, lam, lc, rinf;
  int accept, proceed, ok;
};

__device__ void lm_take_normal(LmState& L, const double (&acc)[45], double rinf) {
  int k = 0;
  for (int a = 0; a < 8; ++a)
    for (int b = a; b < 8; ++b, ++k) L.A[8 * a + b] = L.A[8 * b + a] = acc[k];
  for (int a = 0; a < 8; ++a) L.v[a] = acc[36 + a];
  L.S = acc[44];
  L.rinf = rinf;
}

// Replay, mask, homography, scores, errors, candidates.  One workgroup.
__global__ __launch_bounds__(kBlock) void k_tv_model(TvArgs a, const float* __restrict__ p0,
                                                     const float* __restrict__ p1, const double* __restrict__ models,
                                                     const int* __restrict__ nm, const int* __restrict__ cnt,
                                                     double* __restrict__ head, uint8_t* __restrict__ f_mask,
                                                     double* __restrict__ cand) {
  __shared__ double sh[kWaves * 45];
  __shared__ double s_F[9], s_H[9];
  __shared__ int s_found;
  __shared__ LmState L;
  const int tid = threadIdx.x, n = a.n;
  for (int i = tid; i < hHead; i += kBlock) head[i] = 0.0;
  // ---- RANSACPointSetRegistrator::run's acceptance over the counts
  if (tid == 0) {
    int best = -1, max_good = 0, niters = a.iters;
    for (int it = 0; it < niters && it < a.iters; ++it) {
      const int nr = nm[it];
      for (int r = 0; r < nr; ++r) {
        const int good = cnt[3 * it + r];
        if (good > (max_good > kSub - 1 ? max_good : kSub - 1)) {
          best = 3 * it + r;
          max_good = good;
          // RANSACUpdateNumIters(confidence, outlier ratio, 7, niters)
          const double p = fmin(fmax(a.o.f_confidence, 0.0), 1.0), ep = fmin(fmax(double(n - good) / n, 0.0), 1.0);
          double num = fmax(1.0 - p, DBL_MIN);
          double denom = 1.0 - pow(1.0 - ep, double(kSub));
          if (denom < DBL_MIN) {
            niters = 0;
          } else {
            num = log(num);
            denom = log(denom);
            niters = (denom >= 0 || -num >= niters * (-denom)) ? niters : int(rint(num / denom));
          }
        }
      }
    }
    s_found = best >= 0 ? 1 : 0;
    for (int i = 0; i < 9; ++i) s_F[i] = best >= 0 ? models[size_t(best) * 9 + i] : 0.0;
  }
  __syncthreads();
  const bool found = s_found != 0;
  double F[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = s_F[i];
  // the mask of the accepted (double) model; the scores below read it back
  for (int q = tid; q < n; q += kBlock) f_mask[q] = found && f_inlier(F, p0, p1, q, a.thr32) ? 1 : 0;
  // ---- HomographyEstimatorCallback::runKernel: normalised DLT (M = p0 -> m = p1)
  double c4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int q = tid; q < n; q += kBlock) {
    c4[0] += double(p0[2 * q]); c4[1] += double(p0[2 * q + 1]);
    c4[2] += double(p1[2 * q]); c4[3] += double(p1[2 * q + 1]);
  }
  block_sum<4>(c4, sh);
#pragma unroll
  for (int k = 0; k < 4; ++k) c4[k] = c4[k] / n;
  double s4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int q = tid; q < n; q += kBlock) {
    s4[0] += fabs(double(p0[2 * q]) - c4[0]); s4[1] += fabs(double(p0[2 * q + 1]) - c4[1]);
    s4[2] += fabs(double(p1[2 * q]) - c4[2]); s4[3] += fabs(double(p1[2 * q + 1]) - c4[3]);
  }
  block_sum<4>(s4, sh);
  bool h_ok = fmin(fmin(s4[0], s4[1]), fmin(s4[2], s4[3])) >= DBL_EPSILON;
  if (!(found && h_ok)) return;  // (uniform) no model of either kind: the head stays zero
#pragma unroll
  for (int k = 0; k < 4; ++k) s4[k] = n / s4[k];
  {
    double ltl[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) ltl[k] = 0.0;
    for (int q = tid; q < n; q += kBlock) {
      const double X = (double(p0[2 * q]) - c4[0]) * s4[0], Y = (double(p0[2 * q + 1]) - c4[1]) * s4[1];
      const double x = (double(p1[2 * q]) - c4[2]) * s4[2], y = (double(p1[2 * q + 1]) - c4[3]) * s4[3];
      const double Lx[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x};
      const double Ly[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y};
      int k = 0;
#pragma unroll
      for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j, ++k) ltl[k] += Lx[i] * Lx[j] + Ly[i] * Ly[j];
    }
    block_sum<45>(ltl, sh);
    if (tid == 0) {
      // the eigenvector of the smallest eigenvalue of L^T L (symmetric
      // positive semi-definite: cv::SVD's last singular vector)
      double U[9][9], w[9], Vt[9][9];
      int k = 0;
      for (int i = 0; i < 9; ++i)
        for (int j = i; j < 9; ++j, ++k) U[i][j] = U[j][i] = ltl[k];
      cv_svd_at<9, 9, true>(U, w, Vt);
      const double invHnorm[9] = {1.0 / s4[2], 0, c4[2], 0, 1.0 / s4[3], c4[3], 0, 0, 1};
      const double Hnorm2[9] = {s4[0], 0, -c4[0] * s4[0], 0, s4[1], -c4[1] * s4[1], 0, 0, 1};
      double H0[9], T[9], Hm[9];
      for (int i = 0; i < 9; ++i) H0[i] = Vt[8][i];
      mul3(invHnorm, H0, T);
      mul3(T, Hnorm2, Hm);
      const double sc = 1.0 / Hm[8];
      for (int i = 0; i < 8; ++i) L.x[i] = Hm[i] * sc;
      L.lam = 1.0;
      L.lc = 0.75;
    }
    __syncthreads();
  }
  // ---- cv::LMSolver::run on the 8 parameters (forward transfer error), 10 iterations
  {
    double h[8], acc[45];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = L.x[i];
    double rinf = block_max(h_accumulate<true>(n, p0, p1, h, acc), sh);
    block_sum<45>(acc, sh);
    if (tid == 0) {
      lm_take_normal(L, acc, rinf);
      for (int i = 0; i < 8; ++i) L.D[i] = L.A[9 * i];
    }
    for (int iter = 0;;) {
      if (tid == 0) {
        double Ap[64];
        for (int i = 0; i < 64; ++i) Ap[i] = L.A[i];
        for (int i = 0; i < 8; ++i) Ap[9 * i] += L.D[i] * L.lam;
        L.ok = solve8(Ap, L.v, L.d) ? 1 : 0;
        for (int i = 0; i < 8; ++i) L.xd[i] = L.x[i] - L.d[i];
      }
      __syncthreads();
      if (!L.ok) break;  // (uniform) singular normal equations: keep the current parameters
#pragma unroll
      for (int i = 0; i < 8; ++i) h[i] = L.xd[i];
      double sd1[1];
      h_accumulate<false>(n, p0, p1, h, sd1);
      block_sum<1>(sd1, sh);
      if (tid == 0) {
        const double Sd = sd1[0], S = L.S;
        double dS = 0.0, t = 0.0;
        for (int i = 0; i < 8; ++i) {
          double Ad = 0.0;
          for (int j = 0; j < 8; ++j) Ad += L.A[8 * i + j] * L.d[j];
          dS += L.d[i] * (2 * L.v[i] - Ad);
          t += L.d[i] * L.v[i];
        }
        const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1.0);
        if (R > 0.75) {
          L.lam *= 0.5;
          if (L.lam < L.lc) L.lam = 0.0;
        } else if (R < 0.25) {
          double nu = (Sd - S) / (fabs(t) > DBL_EPSILON ? t : 1.0) + 2;
          nu = fmin(fmax(nu, 2.0), 10.0);
          if (L.lam == 0.0) {
            double maxval = DBL_EPSILON;  // max |diag(A^-1)|
            for (int i = 0; i < 8; ++i) {
              double e[8] = {0, 0, 0, 0, 0, 0, 0, 0}, col[8];
              e[i] = 1.0;
              if (solve8(L.A, e, col)) maxval = fmax(maxval, fabs(col[i]));
            }
            L.lam = L.lc = 1.0 / maxval;
            nu *= 0.5;
          }
          L.lam *= nu;
        }
        L.accept = Sd < S ? 1 : 0;
        if (L.accept)
          for (int i = 0; i < 8; ++i) L.x[i] = L.xd[i];
      }
      __syncthreads();
      if (L.accept) {  // (uniform; h already holds xd)
        rinf = block_max(h_accumulate<true>(n, p0, p1, h, acc), sh);
        block_sum<45>(acc, sh);
        if (tid == 0) lm_take_normal(L, acc, rinf);
      }
      ++iter;
      if (tid == 0) {
        double dinf = 0.0;
        for (int i = 0; i < 8; ++i) dinf = fmax(dinf, fabs(L.d[i]));
        L.proceed = iter < 10 && dinf >= double(FLT_EPSILON) && L.rinf >= double(FLT_EPSILON);
      }
      __syncthreads();
      if (!L.proceed) break;
    }
  }
  // ---- both matrices as the reference's Matx33f holds them
  if (tid == 0) {
    for (int i = 0; i < 8; ++i) s_H[i] = double(float(L.x[i]));
    s_H[8] = 1.0;
    for (int i = 0; i < 9; ++i) s_F[i] = double(float(F[i]));
  }
  __syncthreads();
  double H[9], Hi[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) { H[i] = s_H[i]; F[i] = s_F[i]; }
  inv3(H, Hi);
  // ---- scores (CSfM.cpp:415-469) and average errors
  double sc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // s_h, s_f, errHomo, errFund, inliers
  for (int q = tid; q < n; q += kBlock) {
    const double x0 = p0[2 * q], y0 = p0[2 * q + 1], x1 = p1[2 * q], y1 = p1[2 * q + 1];
    double w = H[6] * x0 + H[7] * y0 + H[8];
    const double fx = (H[0] * x0 + H[1] * y0 + H[2]) / w, fy = (H[3] * x0 + H[4] * y0 + H[5]) / w;
    w = Hi[6] * x1 + Hi[7] * y1 + Hi[8];
    const double bx = (Hi[0] * x1 + Hi[1] * y1 + Hi[2]) / w, by = (Hi[3] * x1 + Hi[4] * y1 + Hi[5]) / w;
    const double e01 = (x1 - fx) * (x1 - fx) + (y1 - fy) * (y1 - fy);
    const double e10 = (x0 - bx) * (x0 - bx) + (y0 - by) * (y0 - by);
    sc[0] += (e01 < a.o.h_score_th ? a.o.h_score_gamma - e01 : 0.0) +
             (e10 < a.o.h_score_th ? a.o.h_score_gamma - e10 : 0.0);
    sc[2] += 0.5 * (sqrt(e01) + sqrt(e10));
    if (f_mask[q]) {  // (written by this thread above)
      const LineTerms t = line_terms(F, x0, y0, x1, y1);
      const double d0 = fabs(t.d0) / sqrt(t.n0), d1 = fabs(t.d1) / sqrt(t.n1);
      sc[1] += (d0 < a.o.f_score_th ? a.o.f_score_gamma - d0 : 0.0) +
               (d1 < a.o.f_score_th ? a.o.f_score_gamma - d1 : 0.0);
      sc[3] += 0.5 * (d0 + d1);
      sc[4] += 1.0;
    }
  }
  block_sum<5>(sc, sh);
  if (tid != 0) return;
  const double s_h = sc[0] / n, s_f = sc[1] / sc[4];
  const double r_h = s_h / (s_h + s_f);
  const int branch = r_h > a.o.h_ratio ? 1 : 2;
  const double avg = branch == 1 ? sc[2] / n : sc[3] / sc[4];
  for (int i = 0; i < 9; ++i) { head[hH + i] = H[i]; head[hF + i] = F[i]; }
  head[hScores] = s_h;
  head[hScores + 1] = s_f;
  head[hAvgErr] = avg;
  head[hBranch] = branch;
  // ---- candidates: R (9) | t (3) each
  int nc = 0;
  double U3[3][3], w3[3], Vt3[3][3], T[9], A3[9];
  if (branch == 2) {
    // E = K1^T F K0: U diag(1, 1, 0) V^T -> R = +-(u2 v1^T - u1 v2^T + u3 v3^T), +-(-u2 v1^T + u1 v2^T + u3 v3^T), t = +-u3
    double K1t[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) K1t[3 * i + j] = a.K1[3 * j + i];
    mul3(K1t, F, T);
    mul3(T, a.K0, A3);
    double E[3][3];
    for (int i = 0; i < 9; ++i) E[i / 3][i % 3] = A3[i];
    cv_svd<3, 3>(E, U3, w3, Vt3);
    double Ra[9], Rb[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double m = U3[1][i] * Vt3[0][j] - U3[0][i] * Vt3[1][j], z = U3[2][i] * Vt3[2][j];
        Ra[3 * i + j] = m + z;
        Rb[3 * i + j] = -m + z;
      }
    const double sa = det3(Ra) < 0 ? -1.0 : 1.0, sb = det3(Rb) < 0 ? -1.0 : 1.0;
    const double tn = sqrt(U3[2][0] * U3[2][0] + U3[2][1] * U3[2][1] + U3[2][2] * U3[2][2]);
    for (int c = 0; c < 4; ++c) {
      for (int i = 0; i < 9; ++i) cand[12 * c + i] = c < 2 ? sa * Ra[i] : sb * Rb[i];
      for (int i = 0; i < 3; ++i) cand[12 * c + 9 + i] = (c & 1 ? -1.0 : 1.0) * (U3[2][i] / tn);
    }
    nc = 4;
  } else {
    // the eight Faugeras candidates of A = K1^-1 H K0 (ORB-SLAM's ReconstructH)
    double K1i[9];
    inv3(a.K1, K1i);
    mul3(K1i, H, T);
    mul3(T, a.K0, A3);
    double Am[3][3];
    for (int i = 0; i < 9; ++i) Am[i / 3][i % 3] = A3[i];
    cv_svd<3, 3>(Am, U3, w3, Vt3);
    const double d1 = w3[0], d2 = w3[1], d3 = w3[2];
    if (!(d1 / d2 < 1.00001 || d2 / d3 < 1.00001)) {
      double Um[9], Vm[9];  // U (columns = left singular vectors), V^T
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { Um[3 * i + j] = U3[j][i]; Vm[3 * i + j] = Vt3[i][j]; }
      const double s = det3(Um) * det3(Vm);
      const double aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
      const double aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
      const double x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
      const double prod = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3));
      const double ast = prod / ((d1 + d3) * d2), ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
      const double asp = prod / ((d1 - d3) * d2), cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
      const double sgn[4] = {1.0, -1.0, -1.0, 1.0};
      for (int c = 0; c < 8; ++c) {
        const int i = c & 3;
        double Rp[9], tp[3], R1[9], R2[9];
        if (c < 4) {
          const double st = sgn[i] * ast;
          const double rp[9] = {ct, 0, -st, 0, 1, 0, st, 0, ct};
          for (int k = 0; k < 9; ++k) Rp[k] = rp[k];
          tp[0] = x1[i] * (d1 - d3); tp[1] = 0.0; tp[2] = -x3[i] * (d1 - d3);
        } else {
          const double sp = sgn[i] * asp;
          const double rp[9] = {cp, 0, sp, 0, -1, 0, sp, 0, -cp};
          for (int k = 0; k < 9; ++k) Rp[k] = rp[k];
          tp[0] = x1[i] * (d1 + d3); tp[1] = 0.0; tp[2] = x3[i] * (d1 + d3);
        }
        mul3(Um, Rp, R1);
        mul3(R1, Vm, R2);
        double t[3];
        for (int k = 0; k < 3; ++k) t[k] = Um[3 * k] * tp[0] + Um[3 * k + 1] * tp[1] + Um[3 * k + 2] * tp[2];
        const double tn = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        for (int k = 0; k < 9; ++k) cand[12 * c + k] = s * R2[k];
        for (int k = 0; k < 3; ++k) cand[12 * c + 9 + k] = t[k] / tn;
      }
      nc = 8;
    }
  }
  head[hNCand] = (avg < a.o.max_repr_err) ? nc : 0;  // the branch fails when its error is too large
}

// One match through one candidate: X, the depths and what the vote needs.
struct TvPoint {
  double X[3], z1, e0, e1, cosp;
  bool finite;
};
__device__ TvPoint tv_point(const TvArgs& a, const double* __restrict__ Rt, double x0, double y0, double x1,
                            double y1) {
  // P0 = K0 [I|0], P1 = K1 [R|t]
  double Pa[12], Pb[12];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Pa[4 * r + c] = a.K0[3 * r + c];
      Pb[4 * r + c] = a.K1[3 * r] * Rt[c] + a.K1[3 * r + 1] * Rt[3 + c] + a.K1[3 * r + 2] * Rt[6 + c];
    }
    Pa[4 * r + 3] = 0.0;
    Pb[4 * r + 3] = a.K1[3 * r] * Rt[9] + a.K1[3 * r + 1] * Rt[10] + a.K1[3 * r + 2] * Rt[11];
  }
  TvPoint p;
  tri_point(Pa, Pb, x0, y0, x1, y1, p.X);
  const double* X = p.X;
  double Xc[3], C1[3], n1[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    Xc[r] = X[0] * Rt[3 * r] + X[1] * Rt[3 * r + 1] + X[2] * Rt[3 * r + 2] + Rt[9 + r];
    C1[r] = -(Rt[r] * Rt[9] + Rt[3 + r] * Rt[10] + Rt[6 + r] * Rt[11]);  // -R^T t
    n1[r] = X[r] - C1[r];
  }
  p.z1 = Xc[2];
  const double u0 = X[0] / X[2] * a.K0[0] + a.K0[2], v0 = X[1] / X[2] * a.K0[4] + a.K0[5];
  const double u1 = Xc[0] / Xc[2] * a.K1[0] + a.K1[2], v1 = Xc[1] / Xc[2] * a.K1[4] + a.K1[5];
  p.e0 = sqrt((u0 - x0) * (u0 - x0) + (v0 - y0) * (v0 - y0));
  p.e1 = sqrt((u1 - x1) * (u1 - x1) + (v1 - y1) * (v1 - y1));
  p.cosp = (X[0] * n1[0] + X[1] * n1[1] + X[2] * n1[2]) /
           (sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]) * sqrt(n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2]));
  p.finite = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
  return p;
}

// The cheirality vote of candidate blockIdx.x over the surviving matches:
// votes [c] = (good points, good points with parallax >= the minimum).
__global__ __launch_bounds__(256) void k_tv_vote(TvArgs a, const float* __restrict__ p0, const float* __restrict__ p1,
                                                 const double* __restrict__ head, const uint8_t* __restrict__ f_mask,
                                                 const double* __restrict__ cand, int* __restrict__ votes) {
  __shared__ int sh[2][4];
  const int c = blockIdx.x;
  if (c >= int(head[hNCand])) {
    if (threadIdx.x == 0) votes[2 * c] = votes[2 * c + 1] = 0;
    return;
  }
  const bool all = int(head[hBranch]) == 1;
  double Rt[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) Rt[i] = cand[12 * c + i];
  int good = 0, par = 0;
  for (int q = threadIdx.x; q < a.n; q += 256) {
    if (!(all || f_mask[q])) continue;
    const TvPoint p = tv_point(a, Rt, p0[2 * q], p0[2 * q + 1], p1[2 * q], p1[2 * q + 1]);
    const bool g = p.finite && p.X[2] > 0 && p.z1 > 0 && p.e0 <= a.o.max_repr_err && p.e1 <= a.o.max_repr_err;
    good += g ? 1 : 0;
    par += g && p.cosp <= a.cos_par ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    good += __shfl_xor(good, off);
    par += __shfl_xor(par, off);
  }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = good; sh[1][threadIdx.x >> 6] = par; }
  __syncthreads();
  if (threadIdx.x == 0) {
    votes[2 * c] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    votes[2 * c + 1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
  }
}

// The winner of the vote, canDecompose, then triangulation and the final
// filter (GeometryUtils::filterMatches on the RANSAC F, CSfM.cpp:922).
__global__ __launch_bounds__(kBlock) void k_tv_final(TvArgs a, const float* __restrict__ p0,
                                                     const float* __restrict__ p1, double* __restrict__ head,
                                                     const uint8_t* __restrict__ f_mask,
                                                     const double* __restrict__ cand, const int* __restrict__ votes,
                                                     double* __restrict__ X, uint8_t* __restrict__ keep) {
  __shared__ double sh[kWaves];
  const int tid = threadIdx.x, n = a.n;
  const int nc = int(head[hNCand]), branch = int(head[hBranch]);
  const bool all = branch == 1;
  // the surviving matches: all (homography: its mask is all ones) or F's inliers
  double ns[1] = {0.0};
  for (int q = tid; q < n; q += kBlock) ns[0] += (all || f_mask[q]) ? 1.0 : 0.0;
  block_sum<1>(ns, sh);
  int best = -1, gb = 0, second = 0;
  for (int c = 0; c < nc; ++c)
    if (votes[2 * c] > gb || best < 0) { best = c; gb = votes[2 * c]; }
  for (int c = 0; c < nc; ++c)
    if (c != best && votes[2 * c] > second) second = votes[2 * c];
  bool ok = best >= 0 && gb > 0;
  if (ok) {
    const double need = fmax(double(a.o.min_good), a.o.min_good_fraction * ns[0]);
    // median parallax >= the minimum: sorted ascending, entry gb / 2 reaches it
    ok = double(gb) >= need && double(second) < a.o.ambiguity_ratio * gb && votes[2 * best + 1] >= gb - gb / 2;
  }
  double Rt[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) Rt[i] = ok ? cand[12 * best + i] : 0.0;
  double F[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = head[hF + i];
  double kept[1] = {0.0};
  for (int q = tid; q < n; q += kBlock) {
    double Xq[3] = {0.0, 0.0, 0.0};
    bool k = false;
    if (ok) {
      const double x0 = p0[2 * q], y0 = p0[2 * q + 1], x1 = p1[2 * q], y1 = p1[2 * q + 1];
      const TvPoint p = tv_point(a, Rt, x0, y0, x1, y1);
      const LineTerms t = line_terms(F, x0, y0, x1, y1);
      const double d0 = fabs(t.d0) / sqrt(t.n0), d1 = fabs(t.d1) / sqrt(t.n1);
      k = (all || f_mask[q]) && p.finite && p.X[2] > 0 && p.z1 > 0 && d0 <= a.o.max_repr_err &&
          d1 <= a.o.max_repr_err;
      Xq[0] = p.X[0]; Xq[1] = p.X[1]; Xq[2] = p.X[2];
    }
    X[3 * size_t(q)] = Xq[0]; X[3 * size_t(q) + 1] = Xq[1]; X[3 * size_t(q) + 2] = Xq[2];
    keep[q] = k ? 1 : 0;
    kept[0] += k ? 1.0 : 0.0;
  }
  block_sum<1>(kept, sh);
  if (tid == 0) {
    head[hBest] = best;
    if (ok) {
      head[hModel] = branch;
      head[hKept] = kept[0];
      for (int i = 0; i < 12; ++i) head[hR + i] = Rt[i];
    }
  }
}

constexpr size_t kHeadBytes = sizeof(double) * hHead;
constexpr size_t out_bytes(size_t m) { return kHeadBytes + sizeof(double) * 3 * m + 2 * m; }

// The calling thread's context on one device (thread_ctx).  The stream first:
// members are destroyed in reverse order, so it goes last.
struct TvCtx {
  Stream stream;
  size_t cap = 0;         // points the three buffers below have room for
  DevArr<float> pts;      // p0 [n][2] | p1 [n][2]
  DevArr<uint8_t> out;    // head | X [n][3] | f_mask [n] | keep [n]
  PinArr<uint8_t> pin;    // pinned staging: the points up, the block down
  DevArr<int> sub;
  int sub_n = -1, sub_iters = -1;
  DevArr<double> models;
  DevArr<int> nm, cnt;
  DevArr<double> cand;
  DevArr<int> votes;
  int init(int /*device*/) {
    if (stream.create(hipStreamNonBlocking) != hipSuccess) return fail(SFM_EIO, "hipStreamCreate failed");
    auto fixed = [](DevBuf& b, size_t bytes) { return b.reserve(bytes, bytes, nullptr); };
    if (fixed(sub, sizeof(int) * kSub * kTvMaxIters) || fixed(models, sizeof(double) * 27 * kTvMaxIters) ||
        fixed(nm, sizeof(int) * kTvMaxIters) || fixed(cnt, sizeof(int) * 3 * kTvMaxIters) ||
        fixed(cand, sizeof(double) * 12 * kMaxCand) || fixed(votes, sizeof(int) * 2 * kMaxCand))
      return fail(SFM_ENOMEM, "hipMalloc failed");
    return 0;
  }
  // room for n points; the three buffers grow together
  int reserve(size_t n) {
    if (n <= cap) return 0;
    cap = 0;
    const size_t want = std::max<size_t>(n, 1024);
    if (pts.reserve(sizeof(float) * 4 * n, sizeof(float) * 4 * want, stream) ||
        out.reserve(out_bytes(n), out_bytes(want), stream) ||
        pin.reserve(sizeof(float) * 4 * n + out_bytes(n), sizeof(float) * 4 * want + out_bytes(want), stream))
      return fail(SFM_ENOMEM, "hipMalloc failed");
    cap = want;
    return 0;
  }
};

}  // namespace
}  // namespace sfm

using namespace sfm;

extern "C" void sfm_two_view_default_options(sfm_two_view_options* o) {
  if (!o) return;
  o->f_ransac_threshold = 3.84;
  o->f_confidence = 0.99;
  o->h_score_th = 5.99;
  o->h_score_gamma = 5.99;
  o->f_score_th = 3.84;
  o->f_score_gamma = 5.99;
  o->h_ratio = 0.45;
  o->max_repr_err = 7.0;
  o->min_good_fraction = 0.9;
  o->ambiguity_ratio = 0.7;
  o->min_parallax_deg = 1.0;
  o->f_max_iters = 1000;
  o->min_good = 50;
}

extern "C" int sfm_two_view_init(int32_t device, int32_t n, const float* pts0, const float* pts1, const double* K0,
                                 const double* K1, const sfm_two_view_options* opts, int32_t* model, double* H9,
                                 double* F9, uint8_t* f_mask, double* scores, double* avg_err, double* R9, double* t3,
                                 uint8_t* keep, double* X, int32_t* n_kept) {
  SFM_TRACE("sfm_two_view_init");
  if (!model) return fail(SFM_EINVAL, "NULL model");
  *model = 0;
  if (n < 0) return fail(SFM_EINVAL, "negative n");
  if (!K0 || !K1 || (n > 0 && (!pts0 || !pts1))) return fail(SFM_EINVAL, "NULL argument");
  TvArgs a;
  if (opts) a.o = *opts;
  else sfm_two_view_default_options(&a.o);
  const sfm_two_view_options& o = a.o;
  if (o.f_max_iters < 0 || o.f_max_iters > kTvMaxIters) return fail(SFM_EINVAL, "f_max_iters out of range");
  if (!(o.f_confidence > 0.0 && o.f_confidence < 1.0)) return fail(SFM_EINVAL, "f_confidence must lie in (0, 1)");
  const double ov[] = {o.f_ransac_threshold, o.h_score_th, o.h_score_gamma, o.f_score_th, o.f_score_gamma, o.h_ratio,
                       o.max_repr_err, o.min_good_fraction, o.ambiguity_ratio, o.min_parallax_deg};
  for (double v : ov)
    if (!std::isfinite(v)) return fail(SFM_EINVAL, "non-finite option");
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(K0[i]) || !std::isfinite(K1[i])) return fail(SFM_EINVAL, "non-finite intrinsics");
  for (size_t i = 0; i < 2 * size_t(n); ++i)
    if (!std::isfinite(pts0[i]) || !std::isfinite(pts1[i])) return fail(SFM_EINVAL, "non-finite point");
  // the outputs of "no initialisation"
  if (H9) std::memset(H9, 0, sizeof(double) * 9);
  if (F9) std::memset(F9, 0, sizeof(double) * 9);
  if (R9) std::memset(R9, 0, sizeof(double) * 9);
  if (t3) std::memset(t3, 0, sizeof(double) * 3);
  if (scores) scores[0] = scores[1] = 0.0;
  if (avg_err) *avg_err = 0.0;
  if (n_kept) *n_kept = 0;
  if (f_mask && n > 0) std::memset(f_mask, 0, size_t(n));
  if (keep && n > 0) std::memset(keep, 0, size_t(n));
  if (X && n > 0) std::memset(X, 0, sizeof(double) * 3 * size_t(n));
  if (n < kMinPoints) return 0;  // OpenCV's LMedS range: not restated
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SFM_ENODEV, "no device");
  if (hipSetDevice(device) != hipSuccess) return fail(SFM_ENODEV, "hipSetDevice failed");
  int rc = 0;
  TvCtx* c = thread_ctx<TvCtx>(device, &rc);
  if (!c) return rc;
  if ((rc = c->reserve(size_t(n)))) return rc;
  std::memcpy(a.K0, K0, sizeof(a.K0));
  std::memcpy(a.K1, K1, sizeof(a.K1));
  a.n = n;
  a.iters = o.f_max_iters > 0 ? o.f_max_iters : 1;
  a.thr32 = float(o.f_ransac_threshold * o.f_ransac_threshold);
  a.cos_par = std::cos(o.min_parallax_deg * (M_PI / 180.0));
  hipStream_t s = c->stream;
  // ONE upload through the pinned stage (the previous call drained the stream)
  float* pin_pts = c->pin.as<float>();
  uint8_t* pin_out = c->pin + sizeof(float) * 4 * c->cap;
  std::memcpy(pin_pts, pts0, sizeof(float) * 2 * size_t(n));
  std::memcpy(pin_pts + 2 * size_t(n), pts1, sizeof(float) * 2 * size_t(n));
  if (hipMemcpyAsync(c->pts, pin_pts, sizeof(float) * 4 * size_t(n), hipMemcpyHostToDevice, s) != hipSuccess)
    return fail(SFM_EIO, "upload failed");
  const float* d_p0 = c->pts;
  const float* d_p1 = c->pts + 2 * size_t(n);
  double* d_head = c->out.as<double>();
  double* d_X = d_head + hHead;
  uint8_t* d_mask = reinterpret_cast<uint8_t*>(d_X + 3 * size_t(n));
  uint8_t* d_keep = d_mask + n;
  // the subsets depend on (n, bound) alone (cv::RNG(-1) restarts per call)
  if (c->sub_n != n || c->sub_iters != a.iters) {
    k_tv_subsets<<<1, 64, 0, s>>>(n, a.iters, c->sub);
    c->sub_n = n;
    c->sub_iters = a.iters;
  }
  k_tv_seven<<<(a.iters + 63) / 64, 64, 0, s>>>(a.iters, d_p0, d_p1, c->sub, c->models, c->nm);
  k_tv_count<<<3 * a.iters, 256, 0, s>>>(n, d_p0, d_p1, c->models, c->nm, a.thr32, c->cnt);
  k_tv_model<<<1, kBlock, 0, s>>>(a, d_p0, d_p1, c->models, c->nm, c->cnt, d_head, d_mask, c->cand);
  k_tv_vote<<<kMaxCand, 256, 0, s>>>(a, d_p0, d_p1, d_head, d_mask, c->cand, c->votes);
  k_tv_final<<<1, kBlock, 0, s>>>(a, d_p0, d_p1, d_head, d_mask, c->cand, c->votes, d_X, d_keep);
  // ONE download, one synchronisation
  const size_t down = out_bytes(size_t(n));
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(pin_out, c->out, down, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    c->sub_n = -1;
    return fail(SFM_EIO, "two-view kernels failed");
  }
  const double* head = reinterpret_cast<const double*>(pin_out);
  const uint8_t* h_mask = pin_out + kHeadBytes + sizeof(double) * 3 * size_t(n);
  *model = int32_t(head[hModel]);
  if (H9) std::memcpy(H9, head + hH, sizeof(double) * 9);
  if (F9) std::memcpy(F9, head + hF, sizeof(double) * 9);
  if (f_mask) std::memcpy(f_mask, h_mask, size_t(n));
  if (scores) { scores[0] = head[hScores]; scores[1] = head[hScores + 1]; }
  if (avg_err) *avg_err = head[hAvgErr];
  if (R9) std::memcpy(R9, head + hR, sizeof(double) * 9);
  if (t3) std::memcpy(t3, head + hT, sizeof(double) * 3);
  if (keep) std::memcpy(keep, h_mask + n, size_t(n));
  if (X) std::memcpy(X, pin_out + kHeadBytes, sizeof(double) * 3 * size_t(n));
  if (n_kept) *n_kept = int32_t(head[hKept]);
  return 0;
}
