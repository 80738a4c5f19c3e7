// Host side of the device bundle adjuster: the Levenberg-Marquardt
// trust-region loop and the C ABI of include/sfm_amd.h (the problem layout,
// sfm_ba_set_problem, is ba_problem.hip's; the handle they share, ba_handle.h).
//
// The loop restates Ceres' TrustRegionMinimizer + LevenbergMarquardtStrategy
// (the solver behind ceres::Solve at /root/reference/CTracker.cpp:700-701,
// options CTracker.cpp:571-577) step for step: its
// bookkeeping is ba_lm.h's state machine, driven here from the device or from
// the host; the per-iteration arithmetic runs in the kernels of
// ba_kernels.hip / chol_kernels.hip and only ~10 scalars cross PCIe per
// iteration.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <map>

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include <chrono>

#include "sfm_trace.h"
#include "ba_device.h"
#include "ba_setup.h"
#include "ba_common.h"
#include "ba_host_layout.h"
#include "ba_handle.h"
#include "../../include/sfm_amd.h"

namespace {
thread_local std::string g_err;
}  // namespace

void sfm_internal_set_error(const std::string& msg) { g_err = msg; }

#define NCCLCHK(expr)                                                                             \
  do {                                                                                            \
    ncclResult_t r_ = (expr);                                                                     \
    if (r_ != ncclSuccess) return fail(SFM_EIO, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
  } while (0)

using namespace sfm;

// The pinned staging buffer with room for `bytes` (the rule it checks: ba_handle.h).
int stage_reserve(sfm_ba_handle* h, size_t bytes) {
  if (bytes <= h->stage.bytes()) return 0;
  if (h->stage && hipStreamQuery(h->stream) == hipErrorNotReady && hipStreamSynchronize(h->stream) != hipSuccess)
    return fail(SFM_EIO, "stream error before the stage regrows");
  if (h->stage.reserve(bytes, std::max<size_t>({bytes, size_t(1) << 20, 2 * h->stage.bytes()}), nullptr))
    return fail(SFM_ENOMEM, "hipHostMalloc failed (staging buffer)");
  return 0;
}

namespace {

constexpr size_t kParamPrefetchMaxBytes = size_t(1) << 20;  // one-shot solves that prefetch their parameters

// ---- phase timing (HIP events on the solver stream; read at the per-iteration sync)
void mark_begin(sfm_ba_handle* h, int ph) {
  if (!h->profiling) return;
  if (h->ev_used + 2 > int(h->ev.size())) {
    const size_t old = h->ev.size();
    h->ev.resize(old + 256);
    for (size_t i = old; i < h->ev.size(); ++i) (void)h->ev[i].create(hipEventDefault);
  }
  h->ev_marks.push_back({ph, h->ev_used});
  hipEventRecord(h->ev[h->ev_used], h->stream);
  h->ev_used += 2;
}
// ends the last mark begun
void mark_end(sfm_ba_handle* h) {
  if (!h->profiling) return;
  hipEventRecord(h->ev[h->ev_marks.back().second + 1], h->stream);
}
void collect_marks(sfm_ba_handle* h) {
  if (!h->profiling) return;
  for (auto& m : h->ev_marks) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[m.second], h->ev[m.second + 1]) == hipSuccess) {
      h->phase_ms[m.first] += ms;
      h->phase_count[m.first] += 1;
    }
  }
  h->ev_marks.clear();
  h->ev_used = 0;
}

// Compute units of the device: the persistent grids (fused Cholesky) size
// themselves to one workgroup per CU (they also finish when only part of the
// grid is resident: roles go by start order).
int device_cus(int device) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || prop.multiProcessorCount < 2) return 2;
  return prop.multiProcessorCount;
}


// ---- device-driven LM loop ----
// The trust-region bookkeeping is ba_lm.h's (lm_init / lm_decide / lm_post on
// an LmCtl), the same functions the host driver calls; here they run on the
// device so that an unsharded solve enqueues several iterations per host
// synchronisation.  k_lm_decide follows compute_step's reductions; the
// accept copy (cam_new -> cam, X_new -> X: enqueued iterations hold fixed
// pointers, where the host driver swaps them) and the evaluation kernels run
// only when the step was accepted (gate run_eval), k_lm_post completes the
// accepted iteration after its evaluation; compute_step's kernels run only
// while the loop is not done (gate run_step).
__global__ void k_lm_decide(LmCtl* c, const double* __restrict__ scal, sfm_ba_iteration* trace, int cap) {
  lm_decide(c, scal, trace, cap);
}
__global__ void k_lm_post(LmCtl* c, const double* __restrict__ scal, sfm_ba_iteration* trace, int cap) {
  lm_post(c, scal, trace, cap);
}
__global__ void k_lm_init(LmCtl* c, const double* __restrict__ scal) { lm_init(c, scal); }

// A phase's batched reduction fused with the bookkeeping that follows it
// (unsharded device loop: no collective sits between them): every
// workgroup reduces its job (reduce_batch_job, as k_reduce_batch), and the
// last one to finish runs k_lm_decide's (kPost: k_lm_post's) body on the
// reduced scalars -- one launch instead of two, ~4.5 us of dispatch each.
// The hand-off is MI355X_MICROARCH.md "Valid forms" row 1 without fences:
// each workgroup's one storing lane stores its scalars sc1, waits for them
// (vmcnt(0)) and adds to the count; the workgroup whose add returns the last
// value re-reads every scalar through sc1 loads after a barrier.  (Two
// __threadfence()s stood there before -- write-back + invalidate of the XCD
// L2, ~3.5 us each, the second by all 1024 threads.)  The count lives in the
// control block, which the loop's upload zeroes, and the last workgroup
// resets it.  Gated like the reduction: with the phase skipped the
// bookkeeping is a no-op too (run_step = 0 only once done, run_eval = 0).
enum LmTail { kTailDecide = 0, kTailPost = 1, kTailInit = 2 };
// Small problems (C <= 256, few points): the accepted step's copy and camera
// preparation -- k_cam_prep with cam_src, the evaluation's first launch --
// run in the deciding workgroup right after lm_decide, when it accepted the
// step.  Same per-camera arithmetic; the |x|^2 partial is the one-workgroup
// sum (the 12 extra waves add +0.0).  C == 0: not folded.
struct AcceptFold {
  int C;
  int64_t n_x;
  double* cam;
  double* camR;
  double* part_xn;
  const double* cam_src;
  const double* X_src;
  double* X_dst;
};
template <int kTail>
__global__ __launch_bounds__(1024) void k_reduce_batch_lm(const double* __restrict__ partials, int64_t max_blocks,
                                                          ReduceBatch b, double* __restrict__ scal,
                                                          const int* __restrict__ fail, const int* __restrict__ gate,
                                                          LmCtl* c, sfm_ba_iteration* trace, int cap,
                                                          const AcceptFold af) {
  if (gate && *gate == 0) return;
  __shared__ double sh[16];
  __shared__ double sc[kNumScalars + 1];
  __shared__ int last;
  reduce_batch_job(partials, max_blocks, b.job[blockIdx.x], scal, blockIdx.x == 0 ? fail : nullptr, sh, true);
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the storing lane's sc1 stores landed)
    last = atomicAdd(&c->red_count, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  // The bookkeeping runs on an LDS copy of the control block, loaded and
  // stored back by the whole workgroup: its branches read and write the
  // block field by field, one dependent memory round trip each in place.
  __shared__ LmCtl lc;
  static_assert(sizeof(LmCtl) % 4 == 0, "LmCtl is copied as 32-bit words");
  constexpr int kCtlWords = int(sizeof(LmCtl) / 4);
  static_assert(kCtlWords <= 1024, "one word per thread");
  if (threadIdx.x <= kNumScalars)
    sc[threadIdx.x] = __hip_atomic_load(scal + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x < kCtlWords) reinterpret_cast<int*>(&lc)[threadIdx.x] = reinterpret_cast<const int*>(c)[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    lc.red_count = 0;
    if (kTail == kTailPost) lm_post(&lc, sc, trace, cap);
    else if (kTail == kTailInit) lm_init(&lc, sc);
    else lm_decide(&lc, sc, trace, cap);
  }
  __syncthreads();
  if (threadIdx.x < kCtlWords) reinterpret_cast<int*>(c)[threadIdx.x] = reinterpret_cast<const int*>(&lc)[threadIdx.x];
  if (kTail != kTailDecide || af.C == 0 || !lc.run_eval) return;
  for (int64_t i = threadIdx.x; i < af.n_x; i += blockDim.x) af.X_dst[i] = af.X_src[i];
  double xn = 0.0;
  const int cc = threadIdx.x;
  if (cc < af.C) {
    double x6[6];
    for (int k = 0; k < 6; ++k) x6[k] = af.cam_src[6 * cc + k];
    for (int k = 0; k < 6; ++k) af.cam[6 * cc + k] = x6[k];
    const double w[3] = {x6[0], x6[1], x6[2]};
    double R[9], dR[27];
    rotation(w, R, dR);
    double* o = af.camR + size_t(kCamR) * cc;
    for (int i = 0; i < 9; ++i) o[i] = R[i];
    for (int i = 0; i < 27; ++i) o[9 + i] = dR[i];
    for (int k = 0; k < 6; ++k) xn += x6[k] * x6[k];
  }
  const double r = block_reduce(xn, sh, false);
  if (threadIdx.x == 0 && af.part_xn) af.part_xn[0] = r;
}

int allreduce(sfm_ba_handle* h, double* buf, size_t count, ncclRedOp_t op) {
  if (h->host_fn) {
    h->host_buf.resize(count);
    HIPCHK(hipMemcpyAsync(h->host_buf.data(), buf, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->host_fn(h->host_buf.data(), int64_t(count), op == ncclMax ? 1 : 0, h->host_user) != 0)
      return fail(SFM_EIO, "host all-reduce callback failed");
    HIPCHK(hipMemcpyAsync(buf, h->host_buf.data(), count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  }
  if (!h->comm) return 0;
  const double scale = op == ncclSum ? double(h->emulate_ranks) : 1.0;
  // Inside a gated phase of the device LM loop the phase's kernels may return
  // at once, leaving `buf` holding the previous, already reduced values: an
  // in-place collective would sum those again (U_c times the rank count after
  // every rejected step).  So the collective goes out of place and a gated
  // kernel copies the result back.  The packed S image is scratch (its pack
  // and unpack are gated themselves) and stays in place.
  const bool gated = h->d.gate != nullptr && buf != h->d.Spack;
  if (!gated) {
    NCCLCHK(ncclAllReduce(buf, buf, count, ncclDouble, op, h->comm.get(), h->stream));
    if (scale != 1.0) launch_gated_copy(buf, buf, int64_t(count), scale, nullptr, h->stream);
    return 0;
  }
  if (h->ar_tmp.bytes() < count * sizeof(double)) {
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->ar_tmp.reserve(count * sizeof(double), std::max<size_t>(count, 4096) * sizeof(double), nullptr))
      return fail(SFM_ENOMEM, "hipMalloc failed (collective scratch)");
  }
  NCCLCHK(ncclAllReduce(buf, h->ar_tmp, count, ncclDouble, op, h->comm.get(), h->stream));
  launch_gated_copy(h->ar_tmp, buf, int64_t(count), scale, h->d.gate, h->stream);
  return 0;
}

// Host-callback collective of kind SFM_COLL_* on device buffers (D2H, the
// callback, H2D; synchronous).  For a plain all-reduce hook the other two
// are built from it: a broadcast is the sum of the root's buffer and the
// others' zeros (exact), a reduce-scatter the all-reduced segments' own.
int host_collective(sfm_ba_handle* h, int kind, double* buf, double* out, int64_t count, int arg) {
  const int64_t in_n = kind == SFM_COLL_REDUCE_SCATTER ? count * h->nranks : count;
  h->host_buf.resize(size_t(in_n));
  HIPCHK(hipMemcpyAsync(h->host_buf.data(), buf, sizeof(double) * size_t(in_n), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int rc = 0;
  double* res = h->host_buf.data();
  if (h->coll_fn) {
    if (kind == SFM_COLL_REDUCE_SCATTER) {
      h->host_buf2.resize(size_t(count));
      res = h->host_buf2.data();
    }
    rc = h->coll_fn(kind, h->host_buf.data(), res, count, arg, h->coll_user);
  } else if (kind == SFM_COLL_BROADCAST) {
    if (h->rank != arg) std::fill(h->host_buf.begin(), h->host_buf.end(), 0.0);
    rc = h->host_fn(h->host_buf.data(), count, 0, h->host_user);
  } else if (kind == SFM_COLL_REDUCE_SCATTER) {
    rc = h->host_fn(h->host_buf.data(), in_n, 0, h->host_user);
    res = h->host_buf.data() + size_t(h->rank) * size_t(count);
  } else {
    rc = h->host_fn(h->host_buf.data(), count, arg, h->host_user);
  }
  if (rc != 0) return fail(SFM_EIO, "host collective callback failed");
  HIPCHK(hipMemcpyAsync(kind == SFM_COLL_REDUCE_SCATTER ? out : buf, res, sizeof(double) * size_t(count),
                        hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int broadcast(sfm_ba_handle* h, double* buf, int64_t count, int root) {
  if (h->host_fn || h->coll_fn) return host_collective(h, SFM_COLL_BROADCAST, buf, nullptr, count, root);
  if (!h->comm) return 0;
  NCCLCHK(ncclBroadcast(buf, buf, size_t(count), ncclDouble, root, h->comm.get(), h->stream));
  return 0;
}

int reduce_scatter(sfm_ba_handle* h, double* send, double* recv, int64_t count) {
  if (h->host_fn || h->coll_fn) return host_collective(h, SFM_COLL_REDUCE_SCATTER, send, recv, count, 0);
  if (!h->comm) return 0;
  NCCLCHK(ncclReduceScatter(send, recv, size_t(count), ncclDouble, ncclSum, h->comm.get(), h->stream));
  return 0;
}

// Sum of count doubles at send over the ranks, into recv on rank `root`.
int reduce_to(sfm_ba_handle* h, double* send, double* recv, int64_t count, int root, hipStream_t st) {
  if (h->host_fn || h->coll_fn) {
    h->host_buf.resize(size_t(count));
    HIPCHK(hipMemcpyAsync(h->host_buf.data(), send, sizeof(double) * size_t(count), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int rc = h->coll_fn ? h->coll_fn(SFM_COLL_REDUCE, h->host_buf.data(), h->host_buf.data(), count, root, h->coll_user)
                        : h->host_fn(h->host_buf.data(), count, 0, h->host_user);  // (an all-reduce: root keeps it)
    if (rc != 0) return fail(SFM_EIO, "host collective callback failed");
    if (h->rank == root) {
      HIPCHK(hipMemcpyAsync(recv, h->host_buf.data(), sizeof(double) * size_t(count), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
  }
  if (!h->comm) return 0;
  NCCLCHK(ncclReduce(send, recv, size_t(count), ncclDouble, ncclSum, root, h->comm.get(), st));
  return 0;
}

// The panel layout of the distributed factor and its buffers (remade when
// the problem size, the panel width or the rank layout changed).
int dist_prepare(sfm_ba_handle* h) {
  DevProblem& d = h->d;
  auto& D = h->dist;
  const int pt = h->dist_pt;
  if (D.send && D.pt == pt && D.nblk == d.nblk && D.n == d.n && D.nranks == h->nranks && D.rank == h->rank) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  for (DevBuf* b : {static_cast<DevBuf*>(&D.send), static_cast<DevBuf*>(&D.recv), static_cast<DevBuf*>(&D.bcast),
                    static_cast<DevBuf*>(&D.off_send)})
    b->reset();
  static_cast<DistLayout&>(D) = DistLayout();  // (the stream and the events stay: made once)
  HIPCHK(D.cstream.create(hipStreamNonBlocking));
  for (Event* e : {&D.ev_packed, &D.ev_free[0], &D.ev_free[1], &D.ev_arrived[0], &D.ev_arrived[1], &D.ev_sent})
    HIPCHK(e->create(hipEventDisableTiming));
  const int np = (d.nblk + pt - 1) / pt, N = h->nranks;
  D.count.assign(size_t(np), 0);
  D.poff.assign(size_t(np), 0);
  for (int J = 0; J < np; ++J) {
    const int c0 = J * pt * kNB, c1 = std::min((J + 1) * pt * kNB, d.n + 1);
    D.count[J] = c1 > c0 ? int64_t(c1 - c0) * (d.n + 1 - c0) : 0;
    D.poff[J] = D.total;
    D.total += D.count[J];
    D.bcast_cap = std::max<int64_t>(D.bcast_cap, D.count[J] + int64_t(pt) * kNB * kNB + 1);
  }
  std::vector<int64_t> os(static_cast<size_t>(np));
  for (int J = 0; J < np; ++J) os[J] = J % N == h->rank ? -1 : D.poff[J];
  auto grab = [](DevBuf& b, size_t bytes) {
    return b.reserve(std::max<size_t>(bytes, 256), std::max<size_t>(bytes, 256), nullptr) == 0;
  };
  if (!grab(D.send, sizeof(double) * size_t(D.total)) || !grab(D.recv, sizeof(double) * size_t(D.total)) ||
      !grab(D.bcast, 2 * sizeof(double) * size_t(D.bcast_cap)) || !grab(D.off_send, sizeof(int64_t) * np))
    return fail(SFM_ENOMEM, "hipMalloc failed (distributed factor buffers)");
  HIPCHK(hipMemcpy(D.off_send, os.data(), sizeof(int64_t) * np, hipMemcpyHostToDevice));
  // the own panels' regions of send stay zero: the owner's partial is
  // updated in place and the others' sum is added just before its factor
  HIPCHK(hipMemsetAsync(D.send, 0, sizeof(double) * size_t(D.total), h->stream));
  while (int(D.ev_red.size()) < np) {
    Event e;
    HIPCHK(e.create(hipEventDisableTiming));
    D.ev_red.push_back(std::move(e));
  }
  D.pt = pt; D.nblk = d.nblk; D.n = d.n; D.nranks = N; D.rank = h->rank;
  return 0;
}

// The reduced camera system's factor, distributed:
// the ranks' partial systems are summed per column panel into its owner (a
// reduce per panel, not one reduce-scatter up front), per panel k its owner
// factors it and broadcasts L (+ its W_k tiles and failure bits), every rank
// applies it to its own later panels; then every rank holds the whole factor
// and back-substitutes (replicated).
// * The owner updates its OWN partial of a panel in place and adds the other
//   ranks' sum (its own region of the send buffer is zero) just before
//   factoring it: the updates are linear, so the panels' reduces can run
//   beside the factorisation instead of ahead of it.
// * Look-ahead: having panel k, the owner of k+1 first updates that panel
//   alone, adds its reduce, factors and packs it, and only then applies
//   panel k to its other panels.
// * Under RCCL the collectives run on a second stream of the handle in the
//   order reduce 0, reduce 1, then per k: broadcast k, reduce k+2 -- so the
//   reduce of a panel lands one step before its owner needs it, and the
//   broadcast of k+1 overlaps the bulk updates (two broadcast buffers,
//   events order each buffer's reuse after its last reader).
// Every panel takes its updates in panel order on every rank count.
int dist_factor_enqueue(sfm_ba_handle* h) {
  SFM_TRACE("sfm:dist_factor");
  DevProblem& d = h->d;
  hipStream_t s = h->stream;
  int rc;
  if ((rc = dist_prepare(h))) return rc;
  auto& D = h->dist;
  const int pt = D.pt, N = h->nranks, me = h->rank, np = int(D.count.size());
  // The broadcasts on a second stream of the handle (the collective stream,
  // two broadcast buffers and the events that order their reuse) only with
  // SFM_DIST_OVERLAP=1.  Its non-owner branches (the wait on ev_free, the
  // unpack, a half reused across owners) have never run with more than one
  // RCCL rank -- no second GPU was ever available to this build, and RCCL
  // takes one rank per GPU -- so the multi-GPU default is the schedule the
  // 2-4-rank host-hook tests run (tests/test_gpu_shards.py), the same order
  // of operations on one stream.  On one rank (RCCL's collectives local) the
  // flag is the one-GPU test of the look-ahead plumbing, tests/test_gpu_scale.py.
  static const bool force_overlap = env_flag("SFM_DIST_OVERLAP");
  const bool overlap = h->comm != nullptr && force_overlap;
  const bool comm = N > 1 || overlap;
  hipStream_t cs = overlap ? D.cstream : s;
  launch_panel_copy(d, kPanelPack, pt, 0, d.n + 1, D.off_send, 0, D.send, s);
  if (overlap) {
    HIPCHK(hipEventRecord(D.ev_sent, s));
    HIPCHK(hipStreamWaitEvent(cs, D.ev_sent, 0));
    // both broadcast halves free from here (the last factor's readers are before this on s)
    HIPCHK(hipEventRecord(D.ev_free[0], s));
    HIPCHK(hipEventRecord(D.ev_free[1], s));
  }
  auto reduce_panel = [&](int k) -> int {
    if (!comm || k >= np) return 0;
    if (int e = reduce_to(h, D.send + D.poff[k], D.recv + D.poff[k], D.count[k], k % N, cs)) return e;
    if (overlap && k % N == me) HIPCHK(hipEventRecord(D.ev_red[k], cs));
    return 0;
  };
  auto geom = [&](int k, int* t0, int* c0, int* c1, int64_t* nw) {
    *t0 = k * pt;
    const int ncols = std::min(pt, d.nblk - *t0);
    *c0 = *t0 * kNB;
    *c1 = *c0 + ncols * kNB;
    *nw = int64_t(ncols) * kNB * kNB;
  };
  auto half = [&](int k) { return D.bcast + size_t(k & 1) * size_t(D.bcast_cap); };
  // the owner's part: the other ranks' sum into its updated partial, factor
  // panel k, pack L + W_k tiles + failure bits
  auto factor_pack = [&](int k) -> int {
    int t0, c0, c1;
    int64_t nw;
    geom(k, &t0, &c0, &c1, &nw);
    if (comm) {
      if (overlap) HIPCHK(hipStreamWaitEvent(s, D.ev_red[k], 0));
      launch_panel_copy(d, kPanelAdd, pt, c0, c1, nullptr, D.poff[k], D.recv, s);
    }
    double* b = half(k);
    launch_cholesky_panel(d, k, pt, ++h->chol_epoch, s);
    launch_panel_copy(d, kPanelPack, pt, c0, c1, nullptr, 0, b, s);
    HIPCHK(hipMemcpyAsync(b + D.count[k], d.invL + size_t(t0) * kNB * kNB, sizeof(double) * size_t(nw),
                          hipMemcpyDeviceToDevice, s));
    launch_fail_slot(d, true, b + D.count[k] + nw, s);
    if (overlap) HIPCHK(hipEventRecord(D.ev_packed, s));
    return 0;
  };
  if ((rc = reduce_panel(0)) || (rc = reduce_panel(1))) return rc;
  if (np > 0 && me == 0 && (rc = factor_pack(0))) return rc;
  for (int k = 0; k < np; ++k) {
    const int owner = k % N;
    int t0, c0, c1;
    int64_t nw;
    geom(k, &t0, &c0, &c1, &nw);
    double* b = half(k);
    const int64_t cnt = D.count[k] + nw + 1;
    if (comm) {
      if (overlap) {
        // the half is packed (owner) / no longer read by panel k-2's unpack
        if (me == owner) HIPCHK(hipStreamWaitEvent(cs, D.ev_packed, 0));
        else HIPCHK(hipStreamWaitEvent(cs, D.ev_free[k & 1], 0));
        NCCLCHK(ncclBroadcast(b, b, size_t(cnt), ncclDouble, owner, h->comm.get(), cs));
        HIPCHK(hipEventRecord(D.ev_arrived[k & 1], cs));
      } else if ((rc = broadcast(h, b, cnt, owner))) {
        return rc;
      }
      if ((rc = reduce_panel(k + 2))) return rc;
      if (overlap) HIPCHK(hipStreamWaitEvent(s, D.ev_arrived[k & 1], 0));
    }
    if (me != owner) {
      launch_panel_copy(d, kPanelUnpack, pt, c0, c1, nullptr, 0, b, s);
      HIPCHK(hipMemcpyAsync(d.invL + size_t(t0) * kNB * kNB, b + D.count[k], sizeof(double) * size_t(nw),
                            hipMemcpyDeviceToDevice, s));
      launch_fail_slot(d, false, b + D.count[k] + nw, s);
      if (overlap) HIPCHK(hipEventRecord(D.ev_free[k & 1], s));
    }
    if (k + 1 < np && (k + 1) % N == me) {
      launch_panel_update(d, k, k + 1, k + 1, pt, N, me, s);  // the next panel first (look-ahead)
      if ((rc = factor_pack(k + 1))) return rc;
    }
    launch_panel_update(d, k, k + 2, INT32_MAX / 2, pt, N, me, s);  // (k+1 is not ours unless updated above)
  }
  return 0;
}

// D2H of the scalar block + stream sync.
int fetch_scalars(sfm_ba_handle* h) {
  HIPCHK(hipMemcpyAsync(h->d.scal_host, h->d.scal, sizeof(double) * (kNumScalars + 1), hipMemcpyDeviceToHost,
                        h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  collect_marks(h);
  return 0;
}

// A phase's closing reduction; in the fused device loop (LmDriver::DeviceFused*) with
// the bookkeeping that follows it: k_lm_decide after compute_step
// (kTailDecide), k_lm_post after an evaluation (kTailPost), k_lm_init after
// the initial one (kTailInit).
void reduce_phase(sfm_ba_handle* h, const ReduceBatch& rb, bool copy_fail, int tail) {
  DevProblem& d = h->d;
  if (h->plan.fused_lm() && rb.n > 0) {
#define SFM_RB_LM(T_)                                                                                      \
  k_reduce_batch_lm<T_><<<rb.n, 1024, 0, h->stream>>>(d.partials, d.max_blocks, rb, d.scal,                 \
                                                      copy_fail ? d.fail : nullptr, d.gate, h->lm_ctl,      \
                                                      h->lm_trace, h->lm_trace_cap, af)
    AcceptFold af{};
    if (tail == kTailPost) SFM_RB_LM(kTailPost);
    else if (tail == kTailInit) SFM_RB_LM(kTailInit);
    else {
      if (h->plan.accept_fold())
        af = AcceptFold{d.C, 3 * int64_t(d.P), d.cam, d.camR,
                        h->plan.cams_var ? d.partials + size_t(kPXNormCam) * d.max_blocks : nullptr,
                        d.cam_new, d.X_new, d.X};
      SFM_RB_LM(kTailDecide);
    }
#undef SFM_RB_LM
    return;
  }
  launch_reduce_batch(d, rb, copy_fail, h->stream);
}

// The evaluation's camera sums and their finalisation on their own (mode 0:
// the unscaled first pass, for the Jacobi scale; mode 1: diagonal and gradient).
int cam_sums_enqueue(sfm_ba_handle* h, int mode) {
  DevProblem& d = h->d;
  hipStream_t s = h->stream;
  mark_begin(h, kPhCamRed);
  if (h->plan.sharded) {
    launch_cam_reduce(d, s);
    if (int rc = allreduce(h, d.Ucam, size_t(kUcam) * d.C, ncclSum)) return rc;
    launch_cam_finalize(d, mode, false, mode == 1, s);
  } else {  // no all-reduce between the two: one launch
    launch_cam_sum_finalize(d, mode, mode == 1, s);
  }
  mark_end(h);
  return 0;
}

// Evaluate cost, Jacobian, Jacobi scale (first call), per-block normal
// equations, LM diagonal and gradient at the current parameters, by the
// solve's plan (ba_plan.h).
int evaluate_enqueue(sfm_ba_handle* h, bool first, bool jacobi_scaling) {
  SFM_TRACE("sfm:evaluate");
  DevProblem& d = h->d;
  const SolvePlan& p = h->plan;
  hipStream_t s = h->stream;
  int rc;
  // constant blocks (STRUCT_ONLY: cameras, POSE_ONLY: points) carry a zero
  // Jacobi scale, so their scaled Jacobian columns vanish; their norms and
  // gradients are left out like Ceres leaves out constant blocks
  if (h->accept_grid > 0) launch_cam_prep_accept(d, p.cams_var, h->accept_grid, s);
  else if (h->accept_grid == 0) launch_cam_prep(d, d.cam, p.cams_var, s);
  // accept_grid < 0: done by the deciding workgroup (AcceptFold)
  // prep_folded: the coming step's preparation rides along (its radius is
  // final here); JacObsPrep: the scaled Jacobian pass is then k_jac_obs_prep's
  // first half, after the point pass below (which reads nothing the Jacobian
  // pass writes)
  const bool jac_first = p.cam_pass == CamPass::Jacobian;
  const bool cams_alone = p.cam_sums == CamSums::SumFinalize || p.cam_sums == CamSums::ReduceAllreduceFinalize;
  if (first && jacobi_scaling) {  // the unscaled pass: the Jacobi scale
    mark_begin(h, kPhJac);
    launch_jacobian(d, false, s);
    mark_end(h);
    if (p.cam_sums == CamSums::InPointPass) {
      mark_begin(h, kPhPtEval);
      launch_point_eval_with_cams(d, 0, false, s);
      mark_end(h);
    } else {
      if ((cams_alone || p.cam_sums == CamSums::SumDiag) && (rc = cam_sums_enqueue(h, 0))) return rc;
      if (p.pts_var) launch_point_eval(d, p.point_pass, 0, false, s);
    }
  }
  if (jac_first) {
    mark_begin(h, kPhJac);
    launch_jacobian(d, true, s);
    mark_end(h);
  }
  if (cams_alone && (rc = cam_sums_enqueue(h, 1))) return rc;
  if (p.cam_sums == CamSums::None) {
    hipMemsetAsync(d.partials + size_t(kPGradCam) * d.max_blocks, 0, sizeof(double) * p.nb_cam, s);
    hipMemsetAsync(d.partials + size_t(kPXNormCam) * d.max_blocks, 0, sizeof(double) * p.nb_cam, s);
  }
  if (p.cam_sums == CamSums::InPointPass) {
    mark_begin(h, kPhPtEval);
    launch_point_eval_with_cams(d, 1, true, s);
    mark_end(h);
  } else if (p.pts_var) {
    mark_begin(h, kPhPtEval);
    launch_point_eval(d, p.point_pass, 1, false, s, p.prep_folded, h->eval_radius);
    mark_end(h);
    if (p.prep_folded) {  // (CamSums::SumDiag: the camera sums follow the observation prep)
      mark_begin(h, kPhPtPrep);
      if (jac_first) launch_obs_prep(d, s);
      else launch_jac_obs_prep(d, s);
      mark_end(h);
      mark_begin(h, kPhCamRed);
      launch_cam_sum_diag(d, h->eval_radius, h->rank == 0, s, p.stage_cams);
      mark_end(h);
      h->cams_staged = p.stage_cams;
    }
    h->prep_fresh = p.prep_folded;
  } else {
    hipMemsetAsync(d.partials + size_t(kPGradPt) * d.max_blocks, 0, sizeof(double) * p.nb_pt, s);
    hipMemsetAsync(d.partials + size_t(kPXNormPt) * d.max_blocks, 0, sizeof(double) * p.nb_pt, s);
  }
  if (d.N == 0) hipMemsetAsync(d.partials + size_t(kPCost) * d.max_blocks, 0, sizeof(double), s);
  if (d.P == 0) {
    hipMemsetAsync(d.partials + size_t(kPGradPt) * d.max_blocks, 0, sizeof(double), s);
    hipMemsetAsync(d.partials + size_t(kPXNormPt) * d.max_blocks, 0, sizeof(double), s);
  }
  ReduceBatch rb;
  rb.add(kPCost, p.nb_cost, 0, kCost);
  rb.add(kPGradCam, p.nb_grad_cam, 1, kGradMaxCam);
  rb.add(kPGradPt, p.nb_pt, 1, kGradMaxPt);
  rb.add(kPXNormCam, p.nb_cam, 0, kXNorm2Cam);
  rb.add(kPXNormPt, p.nb_pt, 0, kXNorm2Pt);
  reduce_phase(h, rb, false, first ? kTailInit : kTailPost);
  if (p.sharded) {
    if ((rc = allreduce(h, d.scal + kCost, 1, ncclSum))) return rc;
    if ((rc = allreduce(h, d.scal + kGradMaxCam, 2, ncclMax))) return rc;
    if ((rc = allreduce(h, d.scal + kXNorm2Pt, 1, ncclSum))) return rc;
  }
  return 0;
}
int evaluate(sfm_ba_handle* h, bool first, bool jacobi_scaling) {
  if (int rc = evaluate_enqueue(h, first, jacobi_scaling)) return rc;
  return fetch_scalars(h);
}

// One trust-region step: factor, Schur, dense Cholesky, back substitution,
// model cost change and candidate cost.
int compute_step_enqueue(sfm_ba_handle* h, double radius) {
  SFM_TRACE("sfm:compute_step");
  DevProblem& d = h->d;
  const SolvePlan& p = h->plan;
  hipStream_t s = h->stream;
  int rc;
  bool cam_done = false;  // the camera step taken by the small-system factor
  // The evaluation prepared this step (prep_folded) unless an
  // unsuccessful or invalid step changed the radius since: then the
  // stand-alone kernels redo it.  Both loops know on the host (prep_fresh):
  // the device loop pauses at such a step, so no launch is spent on the
  // stand-alone kernels while every step is accepted.
  const bool redo_prep = !p.prep_folded || !h->prep_fresh;
  // the stand-alone prep: point factor and k_obs_prep_rc, then the diagonal blocks
  auto point_prep = [&] {
    if (!redo_prep) return;
    mark_begin(h, kPhPtPrep);
    launch_point_prep(d, radius, s);
    mark_end(h);
  };
  auto schur_diag = [&] {
    if (redo_prep) launch_schur_diag(d, radius, h->rank == 0, s);
  };
  if (p.mode == SFM_BA_STRUCT_AND_POSE) {
    point_prep();
    mark_begin(h, kPhSchur);
    if (p.prep_folded) {  // (never a block-per-workgroup system: launch_schur's two parts)
      schur_diag();
      launch_schur_offdiag(d, p.pair_pass, s, h->cams_staged);
    } else {
      launch_schur(d, p.pair_pass, radius, h->rank == 0, s);
    }
    mark_end(h);
    // (k_schur_diag_sum also wrote the identity padding, y's sentinel and
    // the cleared failure flag; without cameras the separate launch does)
    if (!d.C) launch_pad_init(d, s);
    if (p.dist_factor) {
      mark_begin(h, kPhChol);
      if ((rc = dist_factor_enqueue(h))) return rc;
      mark_end(h);
    } else {
      if (p.pack_allreduce) {
        // all-reduce only the packed upper triangle + rhs (half the ld^2 image)
        launch_pack_upper(d, false, s);
        if ((rc = allreduce(h, d.Spack, packed_size(d.n), ncclSum))) return rc;
        launch_pack_upper(d, true, s);
      }
      mark_begin(h, kPhChol);
      cam_done = launch_cholesky(d, ++h->chol_epoch, s, false, h->rank == 0 ? 1 : 0);
      mark_end(h);
    }
    mark_begin(h, kPhBack);
    launch_backsolve(d, ++h->bs_epoch, s, true);
    mark_end(h);
  } else if (p.mode == SFM_BA_POSE_ONLY) {
    // block-diagonal camera system from the all-reduced U_c (same on every rank)
    launch_cam_solve(d, radius, s);
    // the back substitution reads X from the point records (their factor
    // is unused here: y_p = 0); its bad flags are cleared below
    if (d.P) launch_point_factor(d, radius, s);
    hipMemsetAsync(d.partials + size_t(kPBad) * d.max_blocks, 0, sizeof(double) * p.nb_pt, s);
  } else {
    // STRUCT_ONLY: per-point 3x3 systems only; y_c = 0
    hipMemsetAsync(d.fail, 0, sizeof(int), s);
    if (d.P) {
      mark_begin(h, kPhPtPrep);
      launch_point_factor(d, radius, s);
      mark_end(h);
    }
    hipMemsetAsync(d.ysol, 0, sizeof(double) * 6 * size_t(d.C), s);
  }
  // OnePass (large reduced systems): the back substitution as one point-major
  // pass (k_backsub_pm), which builds its camera records from y itself and
  // takes the camera step in its first workgroup: no k_cam_update launch there
  // (cam_done: a one-workgroup factor, never such a system)
  if (!cam_done && p.backsub != Backsub::OnePass) launch_cam_update(d, h->rank == 0 && p.cams_var, s);
  mark_begin(h, kPhBacksub);
  launch_point_backsub(d, p.backsub, s, p.cams_var, p.pts_var, h->rank == 0 && p.cams_var);
  mark_end(h);
  if (d.P == 0) {
    const int slots[] = {kPModel, kPModelPt, kPNewCost, kPStepPt, kPBadBack, kPBad};
    for (int sl : slots) hipMemsetAsync(d.partials + size_t(sl) * d.max_blocks, 0, sizeof(double), s);
  }
  if (h->rank != 0 || !p.cams_var)
    hipMemsetAsync(d.partials + size_t(kPStepCam) * d.max_blocks, 0, sizeof(double) * p.nb_cam, s);
  // (nb_obs: the grid of k_backsub_a_rc / k_backsub_c, nb_back: of k_backsub_b;
  // k_backsub_pm: every partial per 256-point block)
  ReduceBatch rb;
  rb.add(kPModel, p.nb_obs, 0, kModelChange);
  rb.add(kPNewCost, p.nb_obs, 0, kNewCost);
  rb.add(kPStepPt, p.nb_back, 0, kStep2Pt);
  rb.add(kPStepCam, p.nb_cam, 0, kStep2Cam);
  // bad-step flags: max over point_prep, cam_update and backsub partials
  rb.add(kPBad, p.nb_pt, 1, kBadStep);
  rb.add(kPBadCam, p.nb_cam, 1, kBadCam);
  rb.add(kPBadBack, p.nb_back, 1, kBadBack);
  rb.add(kPModelPt, p.nb_back, 0, kModelChangePt);
  // ... and the Cholesky failure flag (an int) into the slot after the scalars
  reduce_phase(h, rb, true, kTailDecide);
  if (p.sharded) {
    if ((rc = allreduce(h, d.scal + kModelChange, 4, ncclSum))) return rc;  // model, new cost, step pt, step cam
    if ((rc = allreduce(h, d.scal + kBadStep, 4, ncclMax))) return rc;
    if ((rc = allreduce(h, d.scal + kModelChangePt, 1, ncclSum))) return rc;
  }
  return 0;
}
int compute_step(sfm_ba_handle* h, double radius) {
  if (int rc = compute_step_enqueue(h, radius)) return rc;
  return fetch_scalars(h);
}

// Ceres 1.12 Solver::Options::IsValid (CommonOptionsAreValid +
// TrustRegionOptionsAreValid): ceres::Solve refuses options that fail these
// (the reference only sets linear_solver_type, CTracker.cpp:571-577).
// Returns the offending rule, or nullptr.
const char* invalid_option(const sfm_ba_options& o) {
  if (!(o.max_num_iterations >= 0)) return "max_num_iterations >= 0";
  if (!(o.max_num_consecutive_invalid_steps >= 0)) return "max_num_consecutive_invalid_steps >= 0";
  if (!(o.function_tolerance >= 0)) return "function_tolerance >= 0";
  if (!(o.gradient_tolerance >= 0)) return "gradient_tolerance >= 0";
  if (!(o.parameter_tolerance >= 0)) return "parameter_tolerance >= 0";
  if (!(o.initial_trust_region_radius > 0)) return "initial_trust_region_radius > 0";
  if (!(o.min_trust_region_radius > 0)) return "min_trust_region_radius > 0";
  if (!(o.max_trust_region_radius > 0)) return "max_trust_region_radius > 0";
  if (!(o.min_trust_region_radius <= o.max_trust_region_radius)) return "min_trust_region_radius <= max";
  if (!(o.min_trust_region_radius <= o.initial_trust_region_radius)) return "min_trust_region_radius <= initial";
  if (!(o.initial_trust_region_radius <= o.max_trust_region_radius)) return "initial_trust_region_radius <= max";
  if (!(o.min_relative_decrease >= 0)) return "min_relative_decrease >= 0";
  if (!(o.min_lm_diagonal >= 0)) return "min_lm_diagonal >= 0";
  if (!(o.max_lm_diagonal >= 0)) return "max_lm_diagonal >= 0";
  if (!(o.min_lm_diagonal <= o.max_lm_diagonal)) return "min_lm_diagonal <= max_lm_diagonal";
  return nullptr;
}

// ---- the LM loop's two drivers over ba_lm.h, and what they share ----

// The loop state before the initial evaluation.
LmCtl lm_start(const sfm_ba_handle* h, const sfm_ba_options& opts) {
  LmCtl c;
  std::memset(&c, 0, sizeof(c));
  c.run_step = 1;
  c.radius = opts.initial_trust_region_radius;
  c.decrease_factor = 2.0;
  c.max_iter = opts.max_num_iterations;
  c.max_invalid = opts.max_num_consecutive_invalid_steps;
  c.ftol = opts.function_tolerance;
  c.gtol = opts.gradient_tolerance;
  c.ptol = opts.parameter_tolerance;
  c.max_radius = opts.max_trust_region_radius;
  c.min_radius = opts.min_trust_region_radius;
  c.min_rel_dec = opts.min_relative_decrease;
  c.prep_fold = h->plan.prep_folded ? 1 : 0;
  return c;
}

// The loop paused at an unsuccessful or invalid step (LmCtl::prep_stale): the
// next step redoes its prep for the new radius.  Whether it re-armed the loop.
bool lm_rearm(sfm_ba_handle* h, LmCtl* c) {
  if (!c->prep_stale) return false;
  h->prep_fresh = false;
  c->prep_stale = 0;
  c->run_step = 1;
  return true;
}

// The finished loop's report: its error bits as messages, else the summary's
// counters, termination and costs, and iteration 0's record followed by the
// loop's.  *nonfinite: the initial cost was not finite (an error whose
// summary, a FAILURE, the caller still gets).
template <class Push>
int lm_report(const sfm_ba_options& opts, const LmCtl& c, const sfm_ba_iteration* trace, int cap, sfm_ba_summary* sm,
              Push& push, bool* nonfinite) {
  if (c.error & 4) return fail(SFM_EIO, "Cholesky tile hand-off timed out (persistent grid made no progress)");
  if (c.error & 2) return fail(SFM_EIO, "back-substitution hand-off timed out (persistent grid made no progress)");
  sm->num_jacobian_evaluations++;  // the initial evaluation
  sm->num_residual_evaluations++;
  sm->initial_cost = c.init_cost;
  sm->final_cost = c.cost;
  if (c.error & 8) {
    *nonfinite = true;
    sm->termination_type = SFM_FAILURE;
    return fail(SFM_EIO, "initial residual evaluation is not finite");
  }
  sfm_ba_iteration it0;
  std::memset(&it0, 0, sizeof(it0));
  it0.cost = c.init_cost;
  it0.gradient_max_norm = c.init_grad;
  it0.trust_region_radius = opts.initial_trust_region_radius;
  it0.step_is_valid = 1;
  it0.step_is_successful = 1;
  push(it0);
  const int n_tr = std::min(c.trace_len, cap);
  for (int i = 0; i < n_tr; ++i) push(trace[i]);
  sm->termination_type = c.termination;
  sm->num_iterations = c.iteration;
  sm->num_successful_steps += c.n_succ;
  sm->num_unsuccessful_steps += c.n_unsucc;
  sm->num_invalid_steps += c.n_invalid;
  sm->num_residual_evaluations += c.n_resid;
  sm->num_jacobian_evaluations += c.n_jac;
  sm->num_linear_solves += c.n_lin;
  return 0;
}

// The host driver (a host-callback collective, the distributed factor, whose
// collectives are not gated, or SFM_HOST_LM=1): one phase at a time, each
// ending in fetch_scalars, the decision taken between them.  Its own: the
// per-phase wall times and the pointer swap that makes the candidate current.
template <class Push>
int run_host_lm(sfm_ba_handle* h, const sfm_ba_options& opts, sfm_ba_summary* sm, Push& push, bool* nonfinite) {
  DevProblem& d = h->d;
  const auto t_start = std::chrono::steady_clock::now();
  auto now_s = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
  LmCtl c = lm_start(h, opts);
  std::vector<sfm_ba_iteration> trace(size_t(std::max(1, opts.max_num_iterations + 1)));
  const int cap = int(trace.size());
  const bool jac_scaling = opts.jacobi_scaling != 0;
  int rc;
  double tj = now_s();
  h->eval_radius = c.radius;
  if ((rc = evaluate(h, true, jac_scaling))) return rc;
  sm->jacobian_time_s += now_s() - tj;
  lm_init(&c, d.scal_host);
  while (!c.done) {
    const double tls = now_s();
    if ((rc = compute_step(h, c.radius))) return rc;
    sm->linear_solver_time_s += now_s() - tls;
    lm_decide(&c, d.scal_host, trace.data(), cap);
    lm_rearm(h, &c);
    if (!c.run_eval) continue;
    std::swap(d.cam, d.cam_new);
    std::swap(d.X, d.X_new);
    tj = now_s();
    h->eval_radius = c.radius;  // the next step's: its preparation rides in the evaluation
    if ((rc = evaluate(h, false, jac_scaling))) return rc;
    sm->jacobian_time_s += now_s() - tj;
    lm_post(&c, d.scal_host, trace.data(), cap);
  }
  return lm_report(opts, c, trace.data(), cap, sm, push, nonfinite);
}

// The device driver (every other solve), initial evaluation included: the
// state block lives on the device, initialised there from the initial
// evaluation (k_lm_init: no host round trip before the first iteration),
// iterations enqueued in batches (3, then 2; SFM_LM_BATCH fixes the size), the
// host reads the control block once per batch.  The gated kernels of
// iterations enqueued past the end return at once.  With an RCCL communicator
// the all-reduces are enqueued on the same stream and every rank decides from
// the same reduced scalars.  (Per-phase host times stay 0 here: the phases
// run asynchronously.)
template <class Push>
int run_device_lm(sfm_ba_handle* h, const sfm_ba_options& opts, sfm_ba_summary* sm, Push& push, bool* nonfinite) {
  DevProblem& d = h->d;
  hipStream_t s = h->stream;
  HostTimer timer;
  timer.tag = "solve";
  if (h->lm_ctl.reserve(sizeof(LmCtl), sizeof(LmCtl), nullptr)) return fail(SFM_ENOMEM, "hipMalloc failed (LM control)");
  if (h->lm_ctl_host.reserve(sizeof(LmCtl), sizeof(LmCtl), nullptr))
    return fail(SFM_ENOMEM, "hipHostMalloc failed (LM control)");
  const int cap = std::max(1, opts.max_num_iterations + 1);
  if (h->lm_trace_cap < cap) {
    h->lm_trace_cap = 0;
    if (h->lm_trace.reserve(sizeof(sfm_ba_iteration) * size_t(cap), sizeof(sfm_ba_iteration) * size_t(cap), s))
      return fail(SFM_ENOMEM, "hipMalloc failed (LM trace)");
    h->lm_trace_cap = cap;
  }
  LmCtl& c = *h->lm_ctl_host;
  c = lm_start(h, opts);
  HIPCHK(hipMemcpyAsync(h->lm_ctl, &c, sizeof(LmCtl), hipMemcpyHostToDevice, s));
  // 3 iterations first (a keyframe or C3 solve typically ends there), then 2
  // at a time: each gated iteration past the end still costs its launches
  // (measured per C1 solve: batch 3 0.49 ms, 4 0.52, 6 0.62; host loop 0.54)
  int batch = 3, batch_next = 2;
  if (h->plan.lm_batch) batch = batch_next = h->plan.lm_batch;
  if (opts.max_num_iterations <= 0) batch = 0;  // k_lm_init ends the solve (NO_CONVERGENCE unless converged)
  const bool jac_scaling = opts.jacobi_scaling != 0;
  const int acc_blocks = std::max(1, std::min(1024, blocks_for(6 * int64_t(d.C) + 3 * int64_t(d.P), 256)));
  d.radius_dev = &h->lm_ctl->radius;
  // (LmDriver::DeviceFused*: a phase's reduction and the bookkeeping are one
  // launch, k_reduce_batch_lm)
  const bool unfused = !h->plan.fused_lm();
  // the initial evaluation (Jacobi scaling on first use); its scalars
  // initialise the loop state on the device
  d.gate = nullptr;
  h->eval_radius = c.radius;  // (the kernels read LmCtl::radius)
  int rc = evaluate_enqueue(h, true, jac_scaling);
  if (rc == 0 && unfused) k_lm_init<<<1, 1, 0, s>>>(h->lm_ctl, d.scal);
  while (rc == 0) {
    for (int b = 0; b < batch && rc == 0; ++b) {
      d.gate = &h->lm_ctl->run_step;
      if ((rc = compute_step_enqueue(h, c.radius))) break;
      d.gate = nullptr;
      if (unfused) k_lm_decide<<<1, 1, 0, s>>>(h->lm_ctl, d.scal, h->lm_trace, h->lm_trace_cap);
      d.gate = &h->lm_ctl->run_eval;
      // k_lm_accept's copy inside the evaluation's k_cam_prep, or already
      // done in the deciding workgroup
      h->accept_grid = h->plan.accept_fold() ? -1 : acc_blocks;
      rc = evaluate_enqueue(h, false, jac_scaling);
      h->accept_grid = 0;
      if (rc) break;
      d.gate = nullptr;
      if (unfused) k_lm_post<<<1, 1, 0, s>>>(h->lm_ctl, d.scal, h->lm_trace, h->lm_trace_cap);
    }
    if (rc) break;
    timer.mark("batch enqueued");
    if (h->prefetch_params) {
      if (hipMemcpyAsync(h->param_host, d.cam, sizeof(double) * 6 * size_t(d.C), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipMemcpyAsync(h->param_host + 6 * size_t(d.C), d.X, sizeof(double) * 3 * size_t(d.P), hipMemcpyDeviceToHost,
                         s) != hipSuccess) {
        rc = fail(SFM_EIO, "parameter readback failed");
        break;
      }
    }
    if (hipMemcpyAsync(&c, h->lm_ctl, sizeof(LmCtl), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      rc = fail(SFM_EIO, "LM control readback failed");
      break;
    }
    timer.mark("batch synchronised");
    collect_marks(h);
    if (c.done) break;
    // (paused: the rest of the batch returned at once)
    if (lm_rearm(h, &c) && hipMemcpyAsync(h->lm_ctl, &c, sizeof(LmCtl), hipMemcpyHostToDevice, s) != hipSuccess) {
      rc = fail(SFM_EIO, "LM control upload failed");
      break;
    }
    batch = batch_next;
  }
  d.gate = nullptr;
  d.radius_dev = nullptr;
  if (rc) return rc;
  // (the trace is in pinned host memory, complete at the last batch's synchronisation)
  rc = lm_report(opts, c, h->lm_trace, h->lm_trace_cap, sm, push, nonfinite);
  if (!rc) h->param_host_valid = h->prefetch_params;
  return rc;
}

}  // namespace

extern "C" {

int32_t sfm_abi_version(void) { return SFM_ABI_VERSION; }
const char* sfm_last_error(void) { return g_err.c_str(); }

void sfm_ba_default_options(sfm_ba_options* o) {
  o->max_num_iterations = 50;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
  o->reserved0 = 0;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->min_relative_decrease = 1e-3;
}

int32_t sfm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sfm_ba_create(int32_t device, sfm_ba_handle** out) {
  if (!out) return fail(SFM_EINVAL, "out is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(SFM_ENODEV, "no HIP device visible");
  if (device < 0 || device >= n) return fail(SFM_EINVAL, "device ordinal out of range");
  HIPCHK(hipSetDevice(device));
  auto* h = new sfm_ba_handle();
  h->device = device;
  if (h->stream.create(hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return fail(SFM_EIO, "hipStreamCreate failed");
  }
  h->n_cu = device_cus(device);  // (hipGetDeviceProperties: once, not per set_problem)
  *out = h;
  return 0;
}

int sfm_ba_destroy(sfm_ba_handle* h) {
  if (!h) return 0;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  delete h;
  return 0;
}

int sfm_comm_unique_id(uint8_t out[128]) {
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  std::memcpy(out, &id, 128);
  return 0;
}

int sfm_ba_set_comm(sfm_ba_handle* h, int32_t nranks, int32_t rank, const uint8_t id[128]) {
  if (!h || nranks < 1 || rank < 0 || rank >= nranks) return fail(SFM_EINVAL, "bad communicator arguments");
  HIPCHK(hipSetDevice(h->device));
  h->set_ranks(nranks, rank);
  h->host_fn = nullptr;
  h->coll_fn = nullptr;
  // a one-rank communicator is created too: it runs every collective of the
  // sharded path (identities over one rank), which the one-GPU tests use
  ncclUniqueId uid;
  ncclComm_t c = nullptr;
  std::memcpy(&uid, id, 128);
  NCCLCHK(ncclCommInitRank(&c, nranks, uid, rank));
  h->comm.reset(c);
  h->emulate_ranks = 1;
  if (const char* e = std::getenv("SFM_EMULATE_IDENTICAL_RANKS")) h->emulate_ranks = std::max(1, std::atoi(e));
  return 0;
}

int sfm_ba_set_host_comm(sfm_ba_handle* h, int32_t nranks, int32_t rank, sfm_allreduce_fn fn, void* user) {
  if (!h || nranks < 1 || rank < 0 || rank >= nranks || !fn) return fail(SFM_EINVAL, "bad communicator arguments");
  h->set_ranks(nranks, rank);
  h->host_fn = fn;
  h->host_user = user;
  h->coll_fn = nullptr;
  h->coll_user = nullptr;
  return 0;
}

// An all-reduce hook built from the general one (kind SFM_COLL_ALLREDUCE).
namespace {
int coll_as_allreduce(double* buf, int64_t count, int32_t op, void* user) {
  auto* h = static_cast<sfm_ba_handle*>(user);
  return h->coll_fn(SFM_COLL_ALLREDUCE, buf, buf, count, op, h->coll_user);
}
}  // namespace

int sfm_ba_set_host_collectives(sfm_ba_handle* h, int32_t nranks, int32_t rank, sfm_collective_fn fn, void* user) {
  if (!h || nranks < 1 || rank < 0 || rank >= nranks || !fn) return fail(SFM_EINVAL, "bad communicator arguments");
  h->set_ranks(nranks, rank);
  h->coll_fn = fn;
  h->coll_user = user;
  h->host_fn = coll_as_allreduce;  // the sharded path's all-reduces
  h->host_user = h;
  return 0;
}

int sfm_ba_set_distributed_factor(sfm_ba_handle* h, int32_t panel_tiles) {
  if (!h || panel_tiles < 0 || panel_tiles > 64) return fail(SFM_EINVAL, "panel_tiles must be in [0, 64]");
  h->dist_pt = panel_tiles;
  return 0;
}

int sfm_ba_reset_parameters(sfm_ba_handle* h) {
  if (!h || !h->has_problem) return fail(SFM_EINVAL, "no problem set");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(h->d.cam, h->d.cam0, sizeof(double) * 6 * size_t(h->d.C), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d.X, h->d.X0, sizeof(double) * 3 * size_t(h->d.P), hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

int sfm_ba_get_parameters(sfm_ba_handle* h, double* rot, double* t, double* X) {
  if (!h || !h->has_problem) return fail(SFM_EINVAL, "no problem set");
  HIPCHK(hipSetDevice(h->device));
  const DevProblem& d = h->d;
  // both arrays through the pinned stage (the stream is drained first: the
  // stage may be regrown, and nothing in flight may still use it)
  HIPCHK(hipStreamSynchronize(h->stream));
  StageLayout gl;
  const size_t o_c = gl.add(sizeof(double) * 6 * size_t(d.C)), o_X = gl.add(sizeof(double) * 3 * size_t(d.P));
  const bool stage_x = gl.bytes <= kStageMaxBytes;  // (else X straight into the caller's array)
  if (int rc = stage_reserve(h, stage_x ? gl.bytes : o_X)) return rc;
  const double* cam = reinterpret_cast<const double*>(h->stage + o_c);
  if (d.C) HIPCHK(hipMemcpyAsync(h->stage + o_c, d.cam, sizeof(double) * 6 * size_t(d.C), hipMemcpyDeviceToHost, h->stream));
  if (X && d.P)
    HIPCHK(hipMemcpyAsync(stage_x ? static_cast<void*>(h->stage + o_X) : static_cast<void*>(X), d.X,
                          sizeof(double) * 3 * size_t(d.P), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (X && d.P && stage_x) std::memcpy(X, h->stage + o_X, sizeof(double) * 3 * size_t(d.P));
  for (int c = 0; c < d.C; ++c)
    for (int j = 0; j < 3; ++j) {
      if (rot) rot[3 * c + j] = cam[6 * c + j];
      if (t) t[3 * c + j] = cam[6 * c + 3 + j];
    }
  return 0;
}

int sfm_ba_set_profiling(sfm_ba_handle* h, int32_t on) {
  if (!h) return fail(SFM_EINVAL, "handle is NULL");
  h->profiling = on != 0;
  for (int i = 0; i < kNumPh; ++i) { h->phase_ms[i] = 0; h->phase_count[i] = 0; }
  return 0;
}

int sfm_ba_phase_times(sfm_ba_handle* h, double* ms) {
  if (!h || !ms) return fail(SFM_EINVAL, "bad arguments");
  for (int i = 0; i < kNumPh; ++i) ms[i] = h->phase_ms[i];
  for (int i = 0; i < kNumPh; ++i) ms[kNumPh + i] = h->phase_count[i];
  return 0;
}

int sfm_ba_sync(sfm_ba_handle* h) {
  if (!h) return fail(SFM_EINVAL, "handle is NULL");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int sfm_ba_solve_resident(sfm_ba_handle* h, const sfm_ba_options* opts_in, int32_t mode, sfm_ba_summary* summary,
                          sfm_ba_iteration* trace, int32_t trace_cap, int32_t* trace_len) {
  SFM_TRACE("sfm_ba_solve_resident");
  const auto t_start = std::chrono::steady_clock::now();
  auto now_s = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
  if (!h || !h->has_problem) return fail(SFM_EINVAL, "no problem set");
  sfm_ba_options opts;
  if (opts_in) opts = *opts_in; else sfm_ba_default_options(&opts);
  if (const char* why = invalid_option(opts)) return fail(SFM_EINVAL, std::string("invalid option: ") + why);
  sfm_ba_summary sm;
  std::memset(&sm, 0, sizeof(sm));
  int tl = 0;
  if (trace_len) *trace_len = 0;
  auto push = [&](const sfm_ba_iteration& it) {
    if (trace && tl < trace_cap) trace[tl] = it;
    ++tl;
    if (trace_len) *trace_len = std::min(tl, trace_cap);
  };
  if (mode < 0 || mode > 2 || h->d.N == 0) {
    // the reference adds no residual blocks for other modes (CTracker.cpp:692-693)
    sm.termination_type = SFM_CONVERGENCE;
    if (summary) *summary = sm;
    return 0;
  }
  HIPCHK(hipSetDevice(h->device));
  DevProblem& d = h->d;
  d.min_diag = opts.min_lm_diagonal;
  d.max_diag = opts.max_lm_diagonal;
  if (!opts.jacobi_scaling) {
    std::vector<double> ones(std::max(6 * size_t(d.C), 3 * size_t(d.P)), 1.0);
    HIPCHK(hipMemcpyAsync(d.scale_c, ones.data(), sizeof(double) * 6 * d.C, hipMemcpyHostToDevice, h->stream));
    if (d.P) HIPCHK(hipMemcpyAsync(d.scale_p, ones.data(), sizeof(double) * 3 * d.P, hipMemcpyHostToDevice, h->stream));
  }
  // constant blocks (CTracker.cpp:679-687): zero scale, so the scaled
  // Jacobian columns of the constant side vanish and its step is zero
  if (mode == SFM_BA_STRUCT_ONLY && d.C) HIPCHK(hipMemsetAsync(d.scale_c, 0, sizeof(double) * 6 * d.C, h->stream));
  if (mode == SFM_BA_POSE_ONLY && d.P) HIPCHK(hipMemsetAsync(d.scale_p, 0, sizeof(double) * 3 * d.P, h->stream));
  // which kernels this solve's passes run, and who drives the loop (ba_plan.h)
  read_knobs(&h->knobs, kKnobsSolve);
  h->plan = plan_solve(d.plan, SolveShape{d.C, d.P, d.N_pad, d.xcd_slice_max}, mode, sharded(h),
                       h->host_fn || h->coll_fn, h->dist_pt, h->knobs);
  h->cams_staged = false;
  bool nonfinite = false;
  const int rc = h->plan.lm == LmDriver::Host ? run_host_lm(h, opts, &sm, push, &nonfinite)
                                              : run_device_lm(h, opts, &sm, push, &nonfinite);
  if (rc && !nonfinite) return rc;
  if (!rc) sm.wall_time_s = now_s();
  if (summary) *summary = sm;
  return rc;
}

int sfm_ba_solve(const sfm_ba_options* opts, int32_t mode, int64_t n_obs, const double* obs_uv,
                 const int32_t* cam_idx, const int32_t* pt_idx, int32_t n_cams, const double* K9, double* rot,
                 double* t, int32_t n_pts, double* X, sfm_ba_summary* summary, sfm_ba_iteration* trace,
                 int32_t trace_cap, int32_t* trace_len) {
  SFM_TRACE("sfm_ba_solve");
  if (mode < 0 || mode > 2 || n_obs == 0) {
    if (summary) { std::memset(summary, 0, sizeof(*summary)); summary->termination_type = SFM_CONVERGENCE; }
    if (trace_len) *trace_len = 0;
    return 0;
  }
  int dev = 0;
  hipGetDevice(&dev);
  // One cached handle per device and calling thread: the drop-in is called
  // once per keyframe (CSfM.cpp:259, 970), so the stream, the pinned mirror
  // and (through the pool) the device buffers are created once, not per call
  // (measured at C1: create 1.7 ms + destroy 2.2 ms against a 1.9-ms solve).
  // The cache owns its handles: they are destroyed (stream, pinned mirror,
  // pooled device buffers) when the calling thread exits.
  struct Cached {
    sfm_ba_handle* h = nullptr;
    int init(int dev) { return sfm_ba_create(dev, &h); }
    ~Cached() { sfm_ba_destroy(h); }
  };
  int rc = 0;
  Cached* cached = thread_ctx<Cached>(dev, &rc);
  if (!cached) return rc;
  sfm_ba_handle* h = cached->h;
  rc = sfm_ba_set_problem(h, n_obs, obs_uv, cam_idx, pt_idx, n_cams, K9, rot, t, n_pts, X);
  // small problems: the parameters ride in the solve's last control readback
  const size_t np = 6 * size_t(std::max(0, n_cams)) + 3 * size_t(std::max(0, n_pts));
  if (!rc && np * sizeof(double) <= kParamPrefetchMaxBytes) {
    (void)h->param_host.reserve(np * sizeof(double), std::max<size_t>(np, 4096) * sizeof(double), h->stream);
    h->prefetch_params = h->param_host != nullptr;
  }
  h->param_host_valid = false;
  if (!rc) rc = sfm_ba_solve_resident(h, opts, mode, summary, trace, trace_cap, trace_len);
  h->prefetch_params = false;
  if (!rc && h->param_host_valid) {
    const double* cam = h->param_host;
    for (int c = 0; c < n_cams; ++c)
      for (int j = 0; j < 3; ++j) {
        rot[3 * c + j] = cam[6 * c + j];
        t[3 * c + j] = cam[6 * c + 3 + j];
      }
    if (n_pts) std::memcpy(X, h->param_host + 6 * size_t(n_cams), sizeof(double) * 3 * size_t(n_pts));
    h->param_host_valid = false;
    return 0;
  }
  h->param_host_valid = false;
  if (!rc) rc = sfm_ba_get_parameters(h, rot, t, X);
  return rc;
}

// The record array of the evaluate API (the solve writes no records):
// allocated on first use, kept with the problem.
static int ensure_records(sfm_ba_handle* h) {
  if (h->d.jrec || h->d.N_pad == 0) return 0;
  return hip_rc(SFM_ENOMEM, "hipMalloc", h->pool.take(&h->d.jrec, size_t(kJRec) * size_t(h->d.N_pad), false));
}

int sfm_ba_evaluate(sfm_ba_handle* h, double* cost, double* res, double* jac) {
  SFM_TRACE("sfm_ba_evaluate");
  if (!h || !h->has_problem) return fail(SFM_EINVAL, "no problem set");
  HIPCHK(hipSetDevice(h->device));
  DevProblem& d = h->d;
  int rc;
  if ((rc = ensure_records(h))) return rc;
  launch_cam_prep(d, d.cam, false, h->stream);
  launch_jacobian(d, false, h->stream, true);  // the records are the output
  if (d.N == 0) HIPCHK(hipMemsetAsync(d.partials, 0, sizeof(double), h->stream));
  // the record-writing grid (jac_blocks_rec) wrote the cost partials: the
  // solve's larger grid's extra slots still hold the last solve's partials
  launch_reduce(d, kPCost, d.plan.jac_blocks_rec, 0, kCost, h->stream);
  std::vector<double> rec(size_t(kJRec) * d.N_pad);
  std::vector<int32_t> order(size_t(d.N)), pos(size_t(d.N));
  if (d.N) {
    HIPCHK(hipMemcpyAsync(rec.data(), d.jrec, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(order.data(), d.order, sizeof(int32_t) * order.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(pos.data(), d.pos, sizeof(int32_t) * pos.size(), hipMemcpyDeviceToHost, h->stream));
  }
  double c = 0;
  HIPCHK(hipMemcpyAsync(&c, d.scal + kCost, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (cost) *cost = c;
  for (int64_t q = 0; q < d.N; ++q) {
    const int64_t i = order[q];
    const double* r = &rec[size_t(kJRec) * pos[q]];
    if (res) { res[2 * i] = r[kRes]; res[2 * i + 1] = r[kRes + 1]; }
    if (jac) {
      double* J = jac + 18 * i;
      for (int row = 0; row < 2; ++row) {
        for (int k = 0; k < 6; ++k) J[9 * row + k] = r[kJC + 6 * row + k];
        for (int k = 0; k < 3; ++k) J[9 * row + 6 + k] = r[kJX + 3 * row + k];
      }
    }
  }
  return 0;
}

}  // extern "C"

namespace {
// The bare dense system of order n the factor and the back substitution work
// on (sfm_dist_factor_profile, dense_solve), from owners: S, invL and the
// flags zeroed (cflags and the 8-byte-aligned cticket inside them), ysol, fail.
// (SFM_EIO: what HIPCHK(hipMalloc(...)) gave these entry points)
int alloc_failed(int hip_error) { return hip_rc(SFM_EIO, "hipMalloc", hip_error); }
struct DenseProblem {
  Stream s;  // first: members are destroyed in reverse order, so it goes last
  DevArr<double> S, invL, ysol;
  DevArr<int> fail_word, flags;
  DevProblem d;
  size_t bytes = 0;  // of S
  int init(int device, int n) {
    d.n = n;
    d.ld = ((n + 1 + kNB - 1) / kNB) * kNB;
    d.nblk = d.ld / kNB;
    bytes = sizeof(double) * size_t(d.ld) * d.ld;
    const size_t b_inv = sizeof(double) * size_t(d.nblk) * kNB * kNB;
    const size_t n_pre = d.nblk + 2 * size_t(d.nblk) * d.nblk, b_flag = sizeof(int) * (n_pre + 16);
    HIPCHK(s.create(hipStreamDefault));
    auto fixed = [](DevBuf& b, size_t n_bytes) { return b.reserve(n_bytes, n_bytes, nullptr); };
    int e = 0;
    if ((e = fixed(S, bytes)) || (e = fixed(invL, b_inv)) || (e = fixed(flags, b_flag)) ||
        (e = fixed(ysol, sizeof(double) * d.ld)) || (e = fixed(fail_word, sizeof(int))))
      return alloc_failed(e);
    HIPCHK(hipMemset(invL, 0, b_inv));
    HIPCHK(hipMemset(flags, 0, b_flag));
    HIPCHK(hipMemset(fail_word, 0, sizeof(int)));
    d.S = S; d.invL = invL; d.ysol = ysol; d.fail = fail_word; d.flags = flags;
    d.cflags = flags + d.nblk;
    d.cticket = reinterpret_cast<unsigned long long*>(flags + n_pre);
    if (reinterpret_cast<uintptr_t>(d.cticket) % 8) d.cticket = reinterpret_cast<unsigned long long*>(flags + n_pre + 1);
    d.n_cu = device_cus(device);
    return 0;
  }
};
}  // namespace

extern "C" {

int sfm_dist_factor_profile(int32_t device, int32_t n, int32_t nranks, int32_t panel_tiles, double* fac_ms,
                            double* pack_ms, double* unpack_ms, double* upd_ms, double* misc_ms) {
  if (n <= 0 || nranks < 1 || panel_tiles < 1 || !fac_ms || !pack_ms || !unpack_ms || !upd_ms || !misc_ms)
    return fail(SFM_EINVAL, "bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SFM_ENODEV, "no device");
  HIPCHK(hipSetDevice(device));
  DenseProblem dp;
  if (int rc = dp.init(device, n)) return rc;
  DevProblem& d = dp.d;
  const int pt = panel_tiles, np = (d.nblk + pt - 1) / pt;
  const size_t bytes = dp.bytes;
  hipStream_t s = dp.s;
  double *S = dp.S, *ys = dp.ysol;
  // one panel rectangle (the broadcast buffer) / the whole lower image (the
  // reduce-scatter's send buffer)
  DevArr<double> buf;
  if (int e = buf.reserve(bytes, bytes, nullptr)) return alloc_failed(e);
  HIPCHK(hipMemset(buf, 0, bytes));
  std::vector<Event> ev(4 * size_t(np) + 8);
  for (auto& e : ev) HIPCHK(e.create(hipEventDefault));
  auto el = [&](hipEvent_t a, hipEvent_t b) {
    float m = 0.f;
    (void)hipEventElapsedTime(&m, a, b);
    return double(m);
  };
  // offsets of every panel in a whole-image buffer (the reduce-scatter pack)
  std::vector<int64_t> off(static_cast<size_t>(np));
  int64_t tot = 0;
  for (int J = 0; J < np; ++J) {
    off[J] = tot;
    const int c0 = J * pt * kNB, c1 = std::min((J + 1) * pt * kNB, n + 1);
    tot += c1 > c0 ? int64_t(c1 - c0) * (n + 1 - c0) : 0;
  }
  DevArr<int64_t> doff;
  if (int e = doff.reserve(sizeof(int64_t) * np, sizeof(int64_t) * np, nullptr)) return alloc_failed(e);
  HIPCHK(hipMemcpy(doff, off.data(), sizeof(int64_t) * np, hipMemcpyHostToDevice));
  int epoch = 0;
  for (int rank = 0; rank < nranks; ++rank) {
    launch_spd_fill(S, d.ld, n, 12345u, s);
    if (rank == 0) {  // reduce-scatter pack + unpack of the whole image, the back substitution
      HIPCHK(hipEventRecord(ev[0], s));
      launch_panel_copy(d, kPanelPack, pt, 0, n + 1, doff, 0, buf, s);
      HIPCHK(hipEventRecord(ev[1], s));
      launch_panel_copy(d, kPanelAdd, pt, 0, n + 1, doff, 0, buf, s);
      HIPCHK(hipEventRecord(ev[2], s));
    }
    for (int k = 0; k < np; ++k) {
      const int owner = k % nranks, t0 = k * pt, ncols = std::min(pt, d.nblk - t0);
      const int c0 = t0 * kNB, c1 = c0 + ncols * kNB;
      if (owner != rank) {  // a zero L for the panels this rank receives: its own panels stay SPD
        const int64_t cols = std::min(c1, n + 1) - c0;
        HIPCHK(hipMemsetAsync(buf + tot, 0, sizeof(double) * (cols * (n + 1 - c0) + int64_t(ncols) * kNB * kNB + 1), s));
      }
      HIPCHK(hipEventRecord(ev[8 + 4 * k], s));
      if (owner == rank) {
        launch_cholesky_panel(d, k, pt, ++epoch, s);
        HIPCHK(hipEventRecord(ev[8 + 4 * k + 1], s));
        launch_panel_copy(d, kPanelPack, pt, c0, c1, nullptr, tot, buf, s);
      } else {
        HIPCHK(hipEventRecord(ev[8 + 4 * k + 1], s));
        launch_panel_copy(d, kPanelUnpack, pt, c0, c1, nullptr, tot, buf, s);
      }
      HIPCHK(hipEventRecord(ev[8 + 4 * k + 2], s));
      launch_panel_update(d, k, k + 1, INT32_MAX / 2, pt, nranks, rank, s);
      HIPCHK(hipEventRecord(ev[8 + 4 * k + 3], s));
    }
    if (rank == 0) {
      HIPCHK(hipMemsetAsync(ys, 0xFF, sizeof(double) * d.ld, s));
      HIPCHK(hipEventRecord(ev[3], s));
      launch_backsolve(d, 1, s);
      HIPCHK(hipEventRecord(ev[4], s));
    }
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < np; ++k) {
      const bool own = k % nranks == rank;
      if (own) fac_ms[k] = el(ev[8 + 4 * k], ev[8 + 4 * k + 1]);
      (own ? pack_ms : unpack_ms)[k] = el(ev[8 + 4 * k + 1], ev[8 + 4 * k + 2]);
      upd_ms[size_t(rank) * np + k] = el(ev[8 + 4 * k + 2], ev[8 + 4 * k + 3]);
    }
    if (rank == 0) {
      misc_ms[0] = el(ev[0], ev[1]);  // reduce-scatter pack
      misc_ms[1] = el(ev[1], ev[2]);  // unpack
      misc_ms[2] = el(ev[3], ev[4]);  // back substitution
    }
  }
  int f = 0;
  HIPCHK(hipMemcpy(&f, d.fail, sizeof(int), hipMemcpyDeviceToHost));
  misc_ms[3] = f;
  misc_ms[4] = double(tot);  // doubles of the whole panel image
  return 0;
}

// sfm_dense_spd_solve (panel_tiles == 0: launch_cholesky) and
// sfm_dense_spd_solve_panels (panel_tiles >= 1: the distributed factor's
// device work on one rank, panel by panel: launch_cholesky_panel, then
// launch_panel_update of every later panel, as dist_factor_enqueue and
// sfm_dist_factor_profile chain them); launch_backsolve after either.
static int dense_solve(int32_t device, int32_t n, const double* A, const double* b, double* y, int32_t reps,
                       int32_t panel_tiles, double* ms, int32_t* chol_fail) {
  if (n <= 0 || !A || !b || !y || reps < 1 || panel_tiles < 0) return fail(SFM_EINVAL, "bad arguments");
  // (up to two tiles launch_backsolve leaves the solve to k_chol_small, which the panel factor does not run)
  if (panel_tiles > 0 && (n + 1 + kNB - 1) / kNB <= 2) return fail(SFM_EINVAL, "panel factor: n < 128");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SFM_ENODEV, "no device");
  HIPCHK(hipSetDevice(device));
  DenseProblem dp;
  if (int rc = dp.init(device, n)) return rc;
  DevProblem& d = dp.d;
  // augmented column-major-lower image: (i, j) at j*ld + i, i >= j
  std::vector<double> img(size_t(d.ld) * d.ld, 0.0);
  for (int j = 0; j < n; ++j)
    for (int i = j; i < n; ++i) img[size_t(j) * d.ld + i] = A[size_t(j) * n + i];  // row-major upper (j, i)
  for (int j = 0; j < n; ++j) img[size_t(j) * d.ld + n] = b[j];
  for (int j = n; j < d.ld; ++j) img[size_t(j) * d.ld + j] = 1.0;
  const size_t bytes = dp.bytes;
  hipStream_t s = dp.s;
  double *S = dp.S, *ys = dp.ysol;
  int* fl = dp.fail_word;
  DevArr<double> S0;
  if (int e = S0.reserve(bytes, bytes, nullptr)) return alloc_failed(e);
  HIPCHK(hipMemcpy(S0, img.data(), bytes, hipMemcpyHostToDevice));
  Event e0, e1;
  HIPCHK(e0.create(hipEventDefault));
  HIPCHK(e1.create(hipEventDefault));
  float total = 0.f;
  int pepoch = 0;  // the panels' flag epoch: one per panel launch
  for (int r = 0; r < reps; ++r) {
    HIPCHK(hipMemcpyAsync(S, S0, bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipEventRecord(e0, s));
    if (panel_tiles > 0) {
      HIPCHK(hipMemsetAsync(fl, 0, sizeof(int), s));
      const int np = (d.nblk + panel_tiles - 1) / panel_tiles;
      for (int k = 0; k < np; ++k) {
        launch_cholesky_panel(d, k, panel_tiles, ++pepoch, s);
        launch_panel_update(d, k, k + 1, INT32_MAX / 2, panel_tiles, 1, 0, s);
      }
    } else {
      launch_cholesky(d, r + 1, s);
    }
    launch_backsolve(d, r + 1, s);
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float m = 0.f;
    HIPCHK(hipEventElapsedTime(&m, e0, e1));
    if (r > 0 || reps == 1) total += m;
  }
  int f = 0;
  HIPCHK(hipMemcpy(&f, fl, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(y, ys, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (ms) *ms = total / (reps > 1 ? reps - 1 : 1);
  if (chol_fail) *chol_fail = f;
  return 0;
}

int sfm_dense_spd_solve(int32_t device, int32_t n, const double* A, const double* b, double* y, int32_t reps,
                        double* ms, int32_t* chol_fail) {
  return dense_solve(device, n, A, b, y, reps, 0, ms, chol_fail);
}

int sfm_dense_spd_solve_panels(int32_t device, int32_t n, const double* A, const double* b, double* y,
                               int32_t panel_tiles, int32_t* chol_fail) {
  if (panel_tiles < 1) return fail(SFM_EINVAL, "bad arguments");
  return dense_solve(device, n, A, b, y, 1, panel_tiles, nullptr, chol_fail);
}

int sfm_ba_bench_jacobian(sfm_ba_handle* h, int32_t reps, double* avg_ms) {
  if (!h || !h->has_problem || reps < 1) return fail(SFM_EINVAL, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  DevProblem& d = h->d;
  int rc;
  if ((rc = ensure_records(h))) return rc;
  launch_cam_prep(d, d.cam, false, h->stream);
  Event e0, e1;
  HIPCHK(e0.create(hipEventDefault));
  HIPCHK(e1.create(hipEventDefault));
  launch_jacobian(d, true, h->stream, true);  // warm (the record-writing pass is what is measured)
  HIPCHK(hipEventRecord(e0, h->stream));
  for (int i = 0; i < reps; ++i) launch_jacobian(d, true, h->stream, true);
  HIPCHK(hipEventRecord(e1, h->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  if (avg_ms) *avg_ms = double(ms) / reps;
  return 0;
}

}  // extern "C"
