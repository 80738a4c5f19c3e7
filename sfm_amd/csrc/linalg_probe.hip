// Testing hook (sfm_linalg_probe): the small dense linear algebra of the
// geometry kernels (cv_linalg.h: cv_svd / cv_svd_at / cv_lstsq / qr_solve;
// pnp_kernels.hip: cv_svd12_lanes) run on the device on a batch of problems,
// every output returned, in the two shapes the product runs them:
//   variant 0  one problem per lane, the sequential sweeps, 256-thread
//              workgroups (k_triangulate's launch);
//   variant 1  one problem per wave through the lane-parallel sweeps (the
//              `lds` path of cv_svd / cv_lstsq, N = 4 or 5), launched as
//              k_pnp_epnp is: 192 threads, three waves, wave w on slice w of
//              one __shared__ array of kSvdLds doubles per wave.
// The kernels only read `in` and write `out`.  The probe of the 12x12 lives
// beside cv_svd12_lanes (pnp_kernels.hip: probe_svd12).
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/sfm_amd.h"
#include "cv_linalg.h"
#include "dev_mem.h"

namespace sfm {
int probe_svd12(int batch, const double* d_in, double* d_out, hipStream_t s);  // pnp_kernels.hip

namespace {

template <int M, int N>
__device__ __forceinline__ void load_mat(const double* __restrict__ a, double (&A)[M][N]) {
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) A[r][c] = a[r * N + c];
}
// out: w [N] | U [N][M] (row i = i-th left singular vector) | Vt [N][N]
template <int M, int N>
__device__ __forceinline__ void store_svd(double* __restrict__ o, const double (&U)[N][M], const double (&w)[N],
                                          const double (&Vt)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) o[i] = w[i];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int k = 0; k < M; ++k) o[N + i * M + k] = U[i][k];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int k = 0; k < N; ++k) o[N + N * M + i * N + k] = Vt[i][k];
}

// ---- variant 0: one problem per lane ------------------------------------
template <int M, int N>
__global__ __launch_bounds__(256) void k_probe_svd(int batch, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  double A[M][N], U[N][M], w[N], Vt[N][N];
  load_mat<M, N>(in + size_t(i) * (M * N), A);
  cv_svd<M, N>(A, U, w, Vt);
  store_svd<M, N>(out + size_t(i) * (N + N * M + N * N), U, w, Vt);
}

// cv_svd_at<9, 7, false> as k_tv_seven calls it (no V): out w [7] | U [7][9]
__global__ __launch_bounds__(256) void k_probe_svd_at97(int batch, const double* __restrict__ in,
                                                        double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const double* a = in + size_t(i) * 63;
  double U[7][9], w[7], Vt[7][7];
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int k = 0; k < 9; ++k) U[r][k] = a[k * 7 + r];
  cv_svd_at<9, 7, false>(U, w, Vt);
  double* o = out + size_t(i) * 70;
#pragma unroll
  for (int r = 0; r < 7; ++r) o[r] = w[r];
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int k = 0; k < 9; ++k) o[7 + r * 9 + k] = U[r][k];
}

// in: A [6][N] | b [6]; out: x [N]
template <int N>
__global__ __launch_bounds__(256) void k_probe_lstsq(int batch, const double* __restrict__ in,
                                                     double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const double* a = in + size_t(i) * (6 * N + 6);
  double A[6][N], b[6], x[N];
  load_mat<6, N>(a, A);
#pragma unroll
  for (int r = 0; r < 6; ++r) b[r] = a[6 * N + r];
  cv_lstsq<6, N>(A, b, x);
#pragma unroll
  for (int k = 0; k < N; ++k) out[size_t(i) * N + k] = x[k];
}

// in: A [6][4] | b [6] | x0 [4]; out: x [4] (x0 where qr_solve returns false) | flag
__global__ __launch_bounds__(256) void k_probe_qr(int batch, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const double* a = in + size_t(i) * 34;
  double A[6][4], b[6], x[4];
  load_mat<6, 4>(a, A);
#pragma unroll
  for (int r = 0; r < 6; ++r) b[r] = a[24 + r];
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = a[30 + k];
  const bool ok = qr_solve(A, b, x);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[size_t(i) * 5 + k] = x[k];
  out[size_t(i) * 5 + 4] = ok ? 1.0 : 0.0;
}

// ---- variant 1: one problem per wave, k_pnp_epnp's launch ----------------
template <int N>
__global__ __launch_bounds__(192) void k_probe_svd_wave(int batch, const double* __restrict__ in,
                                                        double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double lds[3][kSvdLds];
  const int w = threadIdx.x >> 6;
  const int i = blockIdx.x * 3 + w;
  if (i >= batch) return;  // (a whole wave: the sweeps synchronise waves, not the workgroup)
  double A[6][N], U[N][6], wv[N], Vt[N][N];
  load_mat<6, N>(in + size_t(i) * (6 * N), A);
  cv_svd<6, N>(A, U, wv, Vt, lds[w]);
  if ((threadIdx.x & 63) == 0) store_svd<6, N>(out + size_t(i) * (N + N * 6 + N * N), U, wv, Vt);
}

template <int N>
__global__ __launch_bounds__(192) void k_probe_lstsq_wave(int batch, const double* __restrict__ in,
                                                          double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double lds[3][kSvdLds];
  const int w = threadIdx.x >> 6;
  const int i = blockIdx.x * 3 + w;
  if (i >= batch) return;
  const double* a = in + size_t(i) * (6 * N + 6);
  double A[6][N], b[6], x[N];
  load_mat<6, N>(a, A);
#pragma unroll
  for (int r = 0; r < 6; ++r) b[r] = a[6 * N + r];
  cv_lstsq<6, N>(A, b, x, lds[w]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) out[size_t(i) * N + k] = x[k];
}

struct OpShape {
  int n_in, n_out;
  bool wave;  // has a variant 1
};
// per problem, doubles in / out (include/sfm_amd.h SFM_LINALG_*)
constexpr OpShape kOps[SFM_LINALG_NUM_OPS] = {
    {9, 3 + 9 + 9, false},        // SVD_3x3
    {16, 4 + 16 + 16, false},     // SVD_4x4
    {81, 9 + 81 + 81, false},     // SVD_9x9
    {18, 3 + 18 + 9, false},      // SVD_6x3
    {24, 4 + 24 + 16, true},      // SVD_6x4
    {30, 5 + 30 + 25, true},      // SVD_6x5
    {63, 7 + 63, false},          // SVD_AT_9x7
    {18 + 6, 3, false},           // LSTSQ_6x3
    {24 + 6, 4, true},            // LSTSQ_6x4
    {30 + 6, 5, true},            // LSTSQ_6x5
    {24 + 6 + 4, 5, false},       // QR_6x4
    {144, 48, true},              // SVD12 (always per wave)
};

}  // namespace
}  // namespace sfm

using namespace sfm;

extern "C" int sfm_linalg_probe(int32_t device, int32_t op, int32_t variant, int32_t batch, const double* in,
                                double* out) {
  if (op < 0 || op >= SFM_LINALG_NUM_OPS) return fail(SFM_EINVAL, "linalg probe: unknown op");
  const OpShape sh = kOps[op];
  if (variant != 0 && variant != 1) return fail(SFM_EINVAL, "linalg probe: variant must be 0 or 1");
  if (variant == 1 && !sh.wave) return fail(SFM_EINVAL, "linalg probe: this op has no per-wave variant");
  if (op == SFM_LINALG_SVD12 && variant != 1) return fail(SFM_EINVAL, "linalg probe: the 12x12 runs per wave only");
  if (batch < 1 || batch > (1 << 20)) return fail(SFM_EINVAL, "linalg probe: batch out of range");
  if (!in || !out) return fail(SFM_EINVAL, "NULL argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SFM_ENODEV, "no device");
  if (hipSetDevice(device) != hipSuccess) return fail(SFM_ENODEV, "hipSetDevice failed");
  const size_t b_in = sizeof(double) * sh.n_in * size_t(batch), b_out = sizeof(double) * sh.n_out * size_t(batch);
  Stream s;  // (first: destroyed after the buffers)
  DevArr<double> d_in, d_out;
  int rc = 0;
  if (s.create(hipStreamDefault) != hipSuccess) return fail(SFM_ENOMEM, "stream creation failed");
  if (d_in.reserve(b_in, b_in, nullptr) || d_out.reserve(b_out, b_out, nullptr))
    rc = fail(SFM_ENOMEM, "device buffer allocation failed");
  if (!rc && (hipMemcpyAsync(d_in, in, b_in, hipMemcpyHostToDevice, s) != hipSuccess ||
              hipMemsetAsync(d_out, 0, b_out, s) != hipSuccess))
    rc = fail(SFM_EIO, "upload failed");
  if (!rc) {
    const dim3 lane_grid((batch + 255) / 256), wave_grid((batch + 2) / 3);
#define PROBE_LANE(K) K<<<lane_grid, 256, 0, s>>>(batch, d_in, d_out)
#define PROBE_WAVE(K) K<<<wave_grid, 192, 0, s>>>(batch, d_in, d_out)
    switch (op) {
      case SFM_LINALG_SVD_3x3: PROBE_LANE((k_probe_svd<3, 3>)); break;
      case SFM_LINALG_SVD_4x4: PROBE_LANE((k_probe_svd<4, 4>)); break;
      case SFM_LINALG_SVD_9x9: PROBE_LANE((k_probe_svd<9, 9>)); break;
      case SFM_LINALG_SVD_6x3: PROBE_LANE((k_probe_svd<6, 3>)); break;
      case SFM_LINALG_SVD_6x4:
        if (variant) PROBE_WAVE(k_probe_svd_wave<4>); else PROBE_LANE((k_probe_svd<6, 4>));
        break;
      case SFM_LINALG_SVD_6x5:
        if (variant) PROBE_WAVE(k_probe_svd_wave<5>); else PROBE_LANE((k_probe_svd<6, 5>));
        break;
      case SFM_LINALG_SVD_AT_9x7: PROBE_LANE(k_probe_svd_at97); break;
      case SFM_LINALG_LSTSQ_6x3: PROBE_LANE(k_probe_lstsq<3>); break;
      case SFM_LINALG_LSTSQ_6x4:
        if (variant) PROBE_WAVE(k_probe_lstsq_wave<4>); else PROBE_LANE(k_probe_lstsq<4>);
        break;
      case SFM_LINALG_LSTSQ_6x5:
        if (variant) PROBE_WAVE(k_probe_lstsq_wave<5>); else PROBE_LANE(k_probe_lstsq<5>);
        break;
      case SFM_LINALG_QR_6x4: PROBE_LANE(k_probe_qr); break;
      default: rc = probe_svd12(batch, d_in, d_out, s); break;
    }
#undef PROBE_LANE
#undef PROBE_WAVE
    if (rc) rc = fail(SFM_EIO, "linalg probe: launch failed");
    else if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, s) != hipSuccess ||
             hipStreamSynchronize(s) != hipSuccess)
      rc = fail(SFM_EIO, "linalg probe failed");
  }
  return rc;
}
