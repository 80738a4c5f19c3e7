// sfm_ba_set_problem: the caller's observation arrays go up as they are, the
// O(N) layout work runs on the device (ba_setup.hip), and the host lays out
// only the C camera runs.  What a problem's size decides -- one of three
// regimes, one of four parameter routes, the pinned stage's regions -- is
// hostlayout::plan_setup's (ba_host_layout.h, checked on the CPU); the passes
// below carry it out, in the order sfm_ba_set_problem reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "sfm_trace.h"
#include "ba_device.h"
#include "ba_setup.h"
#include "ba_common.h"
#include "ba_host_layout.h"
#include "ba_handle.h"
#include "../../include/sfm_amd.h"

using namespace sfm;
using hostlayout::ParamRoute;

namespace {

struct Setup {
  sfm_ba_handle* const h;
  DevProblem& d;
  const hipStream_t s;
  // the caller's arrays
  const int64_t N;
  const int C, P;
  const double* const obs_uv;
  const int32_t *const cam_idx, *const pt_idx;
  const double* const X;
  const hostlayout::SetupPlan plan;
  HostTimer timer;
  int rc = 0;  // of the last failed alloc() / tmp()

  // host side: packed intrinsics and poses (pageable sources of the Side
  // route: they live until set_problem's last synchronisation), the
  // validation's result and counts
  std::vector<double> Kc, cam;
  std::vector<int32_t> cam_cnt;  // [0..2] first bad observation per kind, [4 + c] observations of camera c
  // host-counted problems with few cameras: per camera, its observations per
  // point slice (the 8 XCD slices of k_small_chunks' key p * 8 / P) -- the
  // chunk table's slice sizes follow from them on the host -- and the pair
  // total's estimate (no same-camera duplicates): the small path then needs no
  // round trip before the pair lists
  std::vector<int32_t> cam_slice;
  int64_t pairs_est = 0;
  hostlayout::Runs runs;
  // what d.plan (ba_plan.h: the small path, the wave-major stream, the Schur
  // pass's shape, ...) is made from, filled in as the passes learn it
  ProblemShape shape;

  // device scratch (the pool's) and pieces of resident blobs the setup alone reads
  uint8_t* in_blob = nullptr;
  double* in_uv = nullptr;
  int32_t *in_cam = nullptr, *in_pt = nullptr, *cnt_p = nullptr, *cnt_c = nullptr;
  int32_t* err = nullptr;  // first bad observation (4) | per-camera counts (C + 1)
  uint64_t *k64a = nullptr, *k64b = nullptr;
  uint32_t *k32a = nullptr, *k32b = nullptr;
  int32_t *iota = nullptr, *pt_s = nullptr, *cm_order = nullptr, *perm = nullptr, *d_cam_off = nullptr;
  int4* ch_in = nullptr;
  void* sort_tmp = nullptr;
  size_t sort_bytes = 0;
  int32_t* small_fill = nullptr;  // small path: the scatters' slot counters (P | C), zeroed in the camera-run blob
  int64_t* poff = nullptr;
  const int32_t* pair_order = nullptr;  // the Schur pair lists' emission order (nullptr: point-major)
  int64_t n_pairs = 0;                  // the pair buffer's size: the device's count, or the small path's bound
  int bperm_per = 0;                    // > 0: the XCD block order's group sizes come back with the last synchronisation
  // the wave-major copy of the point-major stream (DevProblem::uv_wm; wanted
  // until its slot total, back with the pair total's round trip, is above the cap)
  int32_t* wm_cnt = nullptr;
  // the pinned mirror's 17-slot tail: the k_schur_pts group sizes (16), then
  // the deferred uv's finite check (slot 16)
  int64_t* grp_host = nullptr;
  int32_t* uv_err_host = nullptr;

  // large problems: uv goes up from a worker thread; it is joined before any
  // return (the copy writes a buffer of this call and reads the caller's array)
  std::atomic<int> uv_state{0};     // 1: uv's copy and event are enqueued, 2: that failed
  std::atomic<int> param_state{0};  // the same for the parameters' copies (by that worker)
  struct Joiner {
    std::thread t;
    void join() {
      if (t.joinable()) t.join();
    }
    ~Joiner() { join(); }  // (declared after the states: joined before they go)
  } worker;

  Setup(sfm_ba_handle* h_, int64_t n_obs, const double* uv, const int32_t* ci, const int32_t* pi, int n_cams,
        int n_pts, const double* X_)
      : h(h_), d(h_->d), s(h_->stream), N(n_obs), C(n_cams), P(n_pts), obs_uv(uv), cam_idx(ci), pt_idx(pi), X(X_),
        plan(hostlayout::plan_setup(n_obs, n_cams, n_pts, n_obs >= kDeferredUvMinObs && env_flag("SFM_SYNC_UV"))),
        cam_cnt(size_t(n_cams) + 4) {}

  template <typename T>
  bool alloc(T*& p, size_t count, bool scratch = false) {  // resident
    return (rc = hip_rc(SFM_ENOMEM, "hipMalloc", h->pool.take(&p, count, scratch))) == 0;
  }
  template <typename T>
  bool tmp(T*& p, size_t count) { return alloc(p, count, true); }  // back to the pool at the end
};

// waves of 64 points (the wave-major stream's woff has one more entry)
size_t wm_waves(int P) { return (size_t(P) + 63) / 64; }

// The problem's plan from what the setup knows so far: after the camera runs
// (the counts that come back from the layouts still open), and again once
// the pair count and the wave-major slot total are in.
void plan_from_shape(Setup& c) { c.d.plan = plan_problem(c.shape, c.h->knobs); }

// Any failure returns through here: the worker joined and both streams idle, the buffers go back to the pool.
struct ProblemGuard {
  Setup& c;
  bool committed = false;
  ~ProblemGuard() {
    if (committed) return;
    c.worker.join();
    c.h->drop_problem({c.h->stream, c.h->ustream});
  }
};

// ---- parameters: Kc | cam | cam0 | X | X0 in one blob ----
void bind_params(Setup& c, uint8_t* blob) {
  c.d.Kc = reinterpret_cast<double*>(blob + c.plan.o_K);
  c.d.cam = reinterpret_cast<double*>(blob + c.plan.o_c);
  c.d.cam0 = reinterpret_cast<double*>(blob + c.plan.o_c0);
  c.d.X = reinterpret_cast<double*>(blob + c.plan.o_X);
  c.d.X0 = reinterpret_cast<double*>(blob + c.plan.o_X0);
}
int alloc_params(Setup& c) {
  uint8_t* pb = nullptr;
  if (!c.alloc(pb, c.plan.pl_bytes)) return c.rc;
  bind_params(c, pb);
  return 0;
}
// the blob's image in the pinned stage: one DMA
void fill_param_stage(const Setup& c, uint8_t* ps) {
  std::memcpy(ps + c.plan.o_K, c.Kc.data(), sizeof(double) * c.Kc.size());
  std::memcpy(ps + c.plan.o_c, c.cam.data(), sizeof(double) * c.cam.size());
  std::memcpy(ps + c.plan.o_c0, c.cam.data(), sizeof(double) * c.cam.size());
  if (c.P) {
    std::memcpy(ps + c.plan.o_X, c.X, sizeof(double) * 3 * size_t(c.P));
    std::memcpy(ps + c.plan.o_X0, c.X, sizeof(double) * 3 * size_t(c.P));
  }
}
int ensure_side_stream(sfm_ba_handle* h) {
  if (h->ustream) return 0;
  HIPCHK(h->ustream.create(hipStreamNonBlocking));
  HIPCHK(h->uev.create(hipEventDisableTiming));
  return 0;
}
// Side route: from the caller's pageable arrays on the side stream, while the
// layout kernels run (the host's staging copies took ~0.5 ms at C3 after the
// layout round trip, with the device idle); the solve stream waits for uev
// in finish_params.  (Also run by the worker thread: no fail() in here.)
bool side_params_copies(Setup& c) {
  const DevProblem& d = c.d;
  hipStream_t u = c.h->ustream;
  const size_t cam_b = sizeof(double) * c.cam.size(), X_b = sizeof(double) * 3 * size_t(c.P);
  return hipMemcpyAsync(d.Kc, c.Kc.data(), sizeof(double) * c.Kc.size(), hipMemcpyHostToDevice, u) == hipSuccess &&
         hipMemcpyAsync(d.cam, c.cam.data(), cam_b, hipMemcpyHostToDevice, u) == hipSuccess &&
         hipMemcpyAsync(d.cam0, d.cam, cam_b, hipMemcpyDeviceToDevice, u) == hipSuccess &&
         (!c.P || (hipMemcpyAsync(d.X, c.X, X_b, hipMemcpyHostToDevice, u) == hipSuccess &&
                   hipMemcpyAsync(d.X0, d.X, X_b, hipMemcpyDeviceToDevice, u) == hipSuccess)) &&
         hipEventRecord(c.h->uev, u) == hipSuccess;
}
int enqueue_side_params(Setup& c) { return side_params_copies(c) ? 0 : fail(SFM_EIO, "parameter upload failed"); }

// ---- the passes ----

// The stage's room, the input blob, the packed intrinsics and poses; the Side
// route's blob, which its copies may reach from the worker thread.
int open_uploads(Setup& c, const double* K9, const double* rot, const double* t) {
  if (int rc = stage_reserve(c.h, c.plan.stage_bytes)) return rc;
  if (!c.tmp(c.in_blob, c.plan.in_bytes)) return c.rc;
  c.in_uv = reinterpret_cast<double*>(c.in_blob + c.plan.o_uv);
  c.in_cam = reinterpret_cast<int32_t*>(c.in_blob + c.plan.o_cam);
  c.in_pt = reinterpret_cast<int32_t*>(c.in_blob + c.plan.o_pt);
  c.Kc.resize(5 * size_t(c.C));
  c.cam.resize(6 * size_t(c.C));
  for (int i = 0; i < c.C; ++i) {
    const double* k = K9 + 9 * size_t(i);
    double* o = &c.Kc[5 * size_t(i)];
    o[0] = k[0]; o[1] = k[1]; o[2] = k[2]; o[3] = k[4]; o[4] = k[5];
    for (int j = 0; j < 3; ++j) { c.cam[6 * i + j] = rot[3 * i + j]; c.cam[6 * i + 3 + j] = t[3 * i + j]; }
  }
  if (c.plan.route == ParamRoute::Side) {
    if (int rc = alloc_params(c)) return rc;
    return ensure_side_stream(c.h);
  }
  return 0;
}

// Deferred uv: the indices are up; uv (two thirds of the bytes) goes up from a
// worker thread on the side stream -- a pageable copy holds its thread until
// the data has left the caller's array -- while this thread lays out the
// indices; k_uv_layout takes it once it has landed.
int start_uv_worker(Setup& c) {
  sfm_ba_handle* h = c.h;
  if (int rc = ensure_side_stream(h)) return rc;
  HIPCHK(h->uev_uv.create(hipEventDisableTiming));
  Setup* cp = &c;
  auto uv_job = [cp]() {
    Setup& c = *cp;
    bool ok = hipSetDevice(c.h->device) == hipSuccess;
    // (Side route, from the worker: the parameters first, 5 MB the solve needs
    // only at its start, off the copy engine before uv's layouts wait on it)
    if (c.plan.route == ParamRoute::Side)
      c.param_state.store(ok && side_params_copies(c) ? 1 : 2, std::memory_order_release);
    ok = ok && hipMemcpyAsync(c.in_uv, c.obs_uv, sizeof(double) * 2 * size_t(c.N), hipMemcpyHostToDevice,
                              c.h->ustream) == hipSuccess &&
         hipEventRecord(c.h->uev_uv, c.h->ustream) == hipSuccess;
    c.uv_state.store(ok ? 1 : 2, std::memory_order_release);
  };
  // (no exception crosses the C ABI: without a thread the copies run here)
  try {
    c.worker.t = std::thread(uv_job);
  } catch (...) {
    uv_job();
  }
  return 0;
}
// the solve stream takes uv once the worker has enqueued its copy
int wait_uv(Setup& c) {
  c.worker.join();
  if (c.uv_state.load(std::memory_order_acquire) != 1) return fail(SFM_EIO, "observation upload failed");
  if (hipStreamWaitEvent(c.s, c.h->uev_uv, 0) != hipSuccess) return fail(SFM_EIO, "observation upload wait failed");
  return 0;
}

// The observation arrays: staged with the host's checks and counts (one DMA
// from the pinned stage), in line from the caller's arrays, or the indices in
// line and uv from the worker.
int upload_inputs(Setup& c) {
  const hostlayout::SetupPlan& pl = c.plan;
  uint8_t* stg = c.h->stage;
  hipStream_t s = c.s;
  const int64_t N = c.N;
  if (pl.host_counts) {
    // k_validate's checks and counts on the host (ba_host_layout.h); the point
    // counts ride in the upload
    hostlayout::check_and_count(N, c.obs_uv, c.cam_idx, c.pt_idx, c.C, c.P, c.C <= kSmallSetupMaxC, c.cam_cnt.data(),
                                reinterpret_cast<int32_t*>(stg + pl.o_pc), &c.cam_slice, &c.pairs_est);
    c.cnt_p = reinterpret_cast<int32_t*>(c.in_blob + pl.o_pc);
    c.timer.mark("host checks + counts");
  } else {
    if (!(c.tmp(c.err, 4 + size_t(c.C) + 1) && c.tmp(c.cnt_p, size_t(c.P) + 1))) return c.rc;
    c.cnt_c = c.err + 4;
  }
  // (host counts ride in this upload, so it goes up even without
  // observations -- the zero counts then reach cnt_p)
  if (pl.stage_in && (N || pl.host_counts)) {
    if (N) {
      std::memcpy(stg + pl.o_uv, c.obs_uv, sizeof(double) * 2 * size_t(N));
      std::memcpy(stg + pl.o_cam, c.cam_idx, sizeof(int32_t) * size_t(N));
      std::memcpy(stg + pl.o_pt, c.pt_idx, sizeof(int32_t) * size_t(N));
    }
    HIPCHK(hipMemcpyAsync(c.in_blob, stg, pl.in_bytes, hipMemcpyHostToDevice, s));
    c.timer.mark("stage copy + upload");
  } else if (N) {
    HIPCHK(hipMemcpyAsync(c.in_cam, c.cam_idx, sizeof(int32_t) * size_t(N), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c.in_pt, c.pt_idx, sizeof(int32_t) * size_t(N), hipMemcpyHostToDevice, s));
    if (pl.deferred_uv) return start_uv_worker(c);
    HIPCHK(hipMemcpyAsync(c.in_uv, c.obs_uv, sizeof(double) * 2 * size_t(N), hipMemcpyHostToDevice, s));
  }
  return 0;
}

// Without host counts: k_validate, and one round trip for the first bad
// observation and the per-camera counts (the host lays out the C camera runs
// and the wavefront chunk table).
int validate_on_device(Setup& c) {
  const bool deferred_uv = c.plan.deferred_uv;
  uint8_t* stg = c.h->stage;
  hipStream_t s = c.s;
  Fill32Set fs;
  fs.add(c.err, 4 * sizeof(int32_t), uint32_t(INT32_MAX));
  fs.add(c.cnt_c, sizeof(int32_t) * (size_t(c.C) + 1), 0);
  fs.add(c.cnt_p, sizeof(int32_t) * (size_t(c.P) + 1), 0);
  launch_fill32(fs, s);
  // (deferred uv: no point counts either -- pt_off comes from the sorted keys)
  launch_validate(c.N, deferred_uv ? nullptr : c.in_uv, c.in_cam, c.in_pt, c.C, c.P, c.err, c.cnt_c,
                  deferred_uv ? nullptr : c.cnt_p, s);
  // the readback lands in the stage after the upload has read it (stream order)
  HIPCHK(hipMemcpyAsync(stg, c.err, sizeof(int32_t) * (size_t(c.C) + 4), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(c.cam_cnt.data(), stg, sizeof(int32_t) * (size_t(c.C) + 4));
  if (deferred_uv && std::min(c.cam_cnt[0], c.cam_cnt[1]) != INT32_MAX) {
    // a bad index: the whole check once uv is up, so the error reported is
    // the first bad observation of any kind, as without the deferral
    if (int rc = wait_uv(c)) return rc;
    launch_validate(c.N, c.in_uv, c.in_cam, c.in_pt, c.C, c.P, c.err, c.cnt_c, c.cnt_p, s);
    HIPCHK(hipMemcpyAsync(stg, c.err, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(c.cam_cnt.data(), stg, sizeof(int32_t) * 4);
  }
  return 0;
}
int report_first_bad_observation(const Setup& c) {
  const int32_t e0 = c.cam_cnt[0], e1 = c.cam_cnt[1], e2 = c.cam_cnt[2];
  const int32_t first = std::min({e0, e1, e2});
  if (first == INT32_MAX) return 0;
  const char* what = first == e0 ? "cam_idx out of range at " : first == e1 ? "pt_idx out of range at "
                                                                               : "non-finite observation at ";
  return fail(SFM_EINVAL, what + std::to_string(first));
}

// Camera runs: camera-major, each camera's run padded to a whole number of
// 64-wide wavefront chunks; the chunk table camera-major (grouped into 8 point
// slices on the device, one per XCD).  And whether the small path lays out.
void camera_runs(Setup& c) {
  DevProblem& d = c.d;
  hostlayout::camera_runs(c.C, c.cam_cnt.data() + 4, &c.runs);
  d.N_pad = c.runs.npad;
  d.n_jchunks = int32_t(c.runs.chunks.size());
  // The plan so far: the Jacobian passes' grids; keyframe-sized problems take
  // the layouts without radix sorts (the same arrays bit for bit) when the
  // host has the counts and the segments fit the small path's bounds; the
  // others want the wave-major copy of the point-major stream
  ProblemShape& sh = c.shape;
  sh.C = c.C;
  sh.P = c.P;
  sh.N = c.N;
  sh.N_pad = d.N_pad;
  sh.n_jchunks = d.n_jchunks;
  sh.host_counts = c.plan.host_counts;
  sh.small_fits = c.plan.host_counts &&
                  hostlayout::small_setup_fits(c.N, c.C, c.P, c.cam_cnt.data() + 4,
                                               reinterpret_cast<const int32_t*>(c.h->stage + c.plan.o_pc));
  plan_from_shape(c);
  c.timer.mark("camera runs (host)");
}

// Resident arrays of the point-major and camera-major layouts, and the
// scratch of the sorts.
int alloc_layouts(Setup& c) {
  DevProblem& d = c.d;
  const size_t N = size_t(c.N), npad = size_t(d.N_pad);
  const int64_t nch = d.n_jchunks;
  const int64_t nmax = std::max<int64_t>({c.N, nch, 1});
  c.sort_bytes = std::max({setup_sort_bytes(c.N, 64), setup_sort_bytes(nmax, 32), setup_sort_bytes(c.P + 1, 1),
                           setup_sort_bytes(c.N + 1, 2), size_t(256)});
  uint8_t* tb = nullptr;
  const bool ok = (c.d.plan.small_setup || c.alloc(d.pt_off, size_t(c.P) + 1)) &&  // (small path: in the camera-run blob)
                  c.alloc(d.order, N) && c.alloc(d.uv_pm, 2 * N) && c.alloc(d.cam_pm, N) && c.alloc(d.cam_obs, npad) &&
                  c.alloc(d.cm_p, npad) && c.alloc(d.jchunks, size_t(std::max(1, d.n_jchunks))) &&
                  c.alloc(d.jgrp, size_t(9)) && c.alloc(d.uv_cm, 2 * npad) && c.alloc(d.pos, N) &&
                  c.tmp(c.k64a, N) && c.tmp(c.k64b, N) && c.tmp(c.k32a, size_t(nmax)) && c.tmp(c.k32b, size_t(nmax)) &&
                  c.tmp(c.iota, size_t(nmax)) && c.tmp(c.pt_s, N) && c.tmp(c.cm_order, N) &&
                  c.tmp(c.perm, size_t(std::max<int64_t>(1, nch))) && c.tmp(tb, c.sort_bytes) &&
                  (!c.d.plan.wave_major || (c.alloc(d.woff, wm_waves(c.P) + 1) && c.tmp(c.wm_cnt, wm_waves(c.P) + 1)));
  c.sort_tmp = tb;
  return ok ? 0 : c.rc;
}

// The host-made camera runs and chunk table in one resident blob, one DMA
// from the stage (the validation readback was consumed above): cam_rng | wcam
// (resident), cam_off | chunks (read by the setup only).
int upload_runs_blob(Setup& c) {
  DevProblem& d = c.d;
  const hostlayout::SetupPlan& pl = c.plan;
  const hostlayout::Runs& r = c.runs;
  const bool small = c.d.plan.small_setup;
  StageLayout il;
  const size_t o_rng = il.add(sizeof(int32_t) * r.cam_rng.size()), o_w = il.add(sizeof(int32_t) * r.wcam.size()),
               o_off = il.add(sizeof(int32_t) * r.cam_off.size()),
               o_ch = il.add(sizeof(hostlayout::Chunk) * r.chunks.size());
  // small path: pt_off (the host's scan of the point counts, resident) and
  // the zeroed slot counters of the point / camera scatters
  const size_t o_poff = small ? il.add(sizeof(int32_t) * (size_t(c.P) + 1)) : 0,
               o_fill = small ? il.add(sizeof(int32_t) * (size_t(c.P) + size_t(c.C))) : 0;
  if (pl.il_base && il.bytes > pl.il_bound) return fail(SFM_EIO, "internal: camera-run blob above its bound");
  if (int rc = stage_reserve(c.h, pl.il_base + il.bytes)) return rc;  // (never regrows with il_base > 0)
  if (pl.route == ParamRoute::Early && pl.il_base + il.bytes > pl.pl_base)
    return fail(SFM_EIO, "internal: stage layout overlap");
  uint8_t* stg = c.h->stage;
  uint8_t* ib = nullptr;
  if (!c.alloc(ib, il.bytes)) return c.rc;
  uint8_t* sb = stg + pl.il_base;
  std::memcpy(sb + o_rng, r.cam_rng.data(), sizeof(int32_t) * r.cam_rng.size());
  std::memcpy(sb + o_w, r.wcam.data(), sizeof(int32_t) * r.wcam.size());
  std::memcpy(sb + o_off, r.cam_off.data(), sizeof(int32_t) * r.cam_off.size());
  if (!r.chunks.empty()) std::memcpy(sb + o_ch, r.chunks.data(), sizeof(hostlayout::Chunk) * r.chunks.size());
  if (small) {
    const int32_t* pc = reinterpret_cast<const int32_t*>(stg + pl.o_pc);
    int32_t* po = reinterpret_cast<int32_t*>(sb + o_poff);
    po[0] = 0;
    for (int p = 0; p < c.P; ++p) po[p + 1] = po[p] + pc[p];
    std::memset(sb + o_fill, 0, sizeof(int32_t) * (size_t(c.P) + size_t(c.C)));
  }
  if (pl.deferred_uv) {
    // uv's 32-MB DMA is on the copy engine now: this blob, on it, would
    // wait behind it and hold up the layouts, so a kernel reads it from
    // the pinned stage instead (il.bytes: 256-B aligned pieces)
    void* sbd = nullptr;
    HIPCHK(hipHostGetDevicePointer(&sbd, sb, 0));
    launch_copy_from_host(ib, sbd, (il.bytes + 15) / 16 * 16, c.s);
  } else {
    HIPCHK(hipMemcpyAsync(ib, sb, il.bytes, hipMemcpyHostToDevice, c.s));
  }
  if (small) {
    d.pt_off = reinterpret_cast<int32_t*>(ib + o_poff);
    c.small_fill = reinterpret_cast<int32_t*>(ib + o_fill);
  }
  d.cam_rng = reinterpret_cast<int32_t*>(ib + o_rng);
  d.wcam = reinterpret_cast<int32_t*>(ib + o_w);
  c.d_cam_off = reinterpret_cast<int32_t*>(ib + o_off);
  c.ch_in = reinterpret_cast<int4*>(ib + o_ch);
  return 0;
}

// Early route: staged behind the camera-run blob and uploaded before the
// layout launches (its host copies overlap the layout kernels).
int upload_params_early(Setup& c) {
  if (int rc = alloc_params(c)) return rc;
  uint8_t* ps = c.h->stage + c.plan.pl_base;
  fill_param_stage(c, ps);
  HIPCHK(hipMemcpyAsync(c.d.Kc, ps, c.plan.pl_bytes, hipMemcpyHostToDevice, c.s));
  return 0;
}

// Small path: the same layouts without radix sorts -- point-major by (point,
// camera, caller index), camera-major by (camera, point-major id), the chunk
// table by slice, the pair counts per block (seg = their exclusive sum,
// seg[n_blk] = the pair total).  No round trip: the pair lists go into a
// buffer of the pair total's bound (every ordered pair of a point's
// observations: twice the estimate), and the chunk table's slice sizes come
// from the host's per-camera slice counts.
int layout_small(Setup& c) {
  DevProblem& d = c.d;
  hipStream_t s = c.s;
  int32_t* small_cnt = nullptr;  // per-block pair counts
  d.n_blk = int64_t(c.C) * (c.C + 1) / 2;
  if (!(c.alloc(d.seg, size_t(d.n_blk) + 1) && c.tmp(small_cnt, std::max<size_t>(1, size_t(d.n_blk))))) return c.rc;
  c.timer.mark("allocs + camera-run blob");
  launch_small_pm(c.N, c.in_pt, c.in_cam, c.in_uv, d.pt_off, c.small_fill, reinterpret_cast<int32_t*>(c.k32a), d.order,
                  d.uv_pm, d.cam_pm, c.pt_s, s);
  launch_small_cm(c.N, c.C, d.cam_pm, c.d_cam_off, c.cm_order, s);
  launch_fill_cm(d.N_pad, d.wcam, d.cam_rng, c.d_cam_off, c.cm_order, c.pt_s, d.uv_pm, d.cm_p, d.uv_cm, d.cam_obs,
                 d.pos, s);
  launch_small_chunks(d.n_jchunks, c.ch_in, c.cm_order, c.pt_s, c.P, d.jchunks, d.jgrp, s);
  launch_small_pairs_count(c.C, d.n_blk, c.d_cam_off, c.cm_order, d.cam_pm, c.pt_s, d.pt_off, small_cnt, d.seg, s);
  c.n_pairs = std::max<int64_t>(1, 2 * c.pairs_est);
  d.xcd_slice_max = hostlayout::small_slice_max(c.C, c.cam_cnt.data() + 4, c.cam_slice);
  c.timer.mark("layout launches");
  return 0;
}

// Sorted path: the layouts by radix sorts, up to the Schur pair counts.
int layout_sorted(Setup& c) {
  DevProblem& d = c.d;
  hipStream_t s = c.s;
  const int64_t N = c.N;
  const int C = c.C, P = c.P, nch = d.n_jchunks;
  const bool deferred_uv = c.plan.deferred_uv;
  c.timer.mark("allocs + camera-run blob");
  // point-major order: stable sort by (point, camera)
  launch_pm_keys(N, c.in_cam, c.in_pt, C, c.k64a, c.iota, s);
  HIPCHK(sort_pairs64(c.sort_tmp, c.sort_bytes, c.k64a, c.k64b, c.iota, d.order, N,
                      uint64_t(std::max(1, P)) * uint64_t(std::max(1, C)) - 1, s));
  launch_gather_pm(N, d.order, deferred_uv ? nullptr : c.in_uv, c.in_cam, c.in_pt, d.uv_pm, d.cam_pm, c.pt_s, c.k32a,
                   c.iota, s);
  if (deferred_uv) launch_pt_off(P, c.k64b, N, C, d.pt_off, s);
  else HIPCHK(exclusive_sum32(c.sort_tmp, c.sort_bytes, c.cnt_p, d.pt_off, int64_t(P) + 1, s));
  if (c.d.plan.wave_major) HIPCHK(launch_wm_off(P, d.pt_off, c.wm_cnt, d.woff, c.sort_tmp, c.sort_bytes, s));
  // camera-major order of the point-major ids: stable sort by camera
  HIPCHK(sort_pairs32(c.sort_tmp, c.sort_bytes, c.k32a, c.k32b, c.iota, c.cm_order, N, uint64_t(std::max(1, C)) - 1,
                      s));
  launch_fill_cm(d.N_pad, d.wcam, d.cam_rng, c.d_cam_off, c.cm_order, c.pt_s, deferred_uv ? nullptr : d.uv_pm, d.cm_p,
                 d.uv_cm, d.cam_obs, d.pos, s);
  // chunk table grouped by point slice (stable: camera-major order kept)
  launch_chunk_keys(nch, c.ch_in, c.cm_order, c.pt_s, P, c.k32a, c.iota, s);
  HIPCHK(sort_pairs32(c.sort_tmp, c.sort_bytes, c.k32a, c.k32b, c.iota, c.perm, nch, 7, s));
  launch_chunk_gather(nch, c.perm, c.ch_in, c.k32b, d.jchunks, d.jgrp, s);
  // Schur pair counts: the second (and last) round trip
  int64_t* pcnt = nullptr;
  if (!(c.tmp(pcnt, size_t(N) + 1) && c.tmp(c.poff, size_t(N) + 1))) return c.rc;
  // (point-major emission: the same lists; SFM_PAIRS_CM=1 emits in camera-major order)
  c.pair_order = env_flag("SFM_PAIRS_CM") ? c.cm_order : nullptr;
  launch_pair_count(N, c.pair_order, d.cam_pm, c.pt_s, d.pt_off, pcnt, s);
  HIPCHK(exclusive_sum64(c.sort_tmp, c.sort_bytes, pcnt, c.poff, N + 1, s));
  return 0;
}

// Sorted path: the pair total and the 8 slices' chunk offsets (the
// observation passes size their grids by the largest slice, obs_xcd_blocks)
// on their way into the stage: stream order puts them after the uploads that
// read it.
int enqueue_total_readback(Setup& c) {
  uint8_t* stg = c.h->stage;
  if (!c.plan.deferred_uv) {
    HIPCHK(hipMemcpyAsync(stg, c.poff + c.N, sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
    HIPCHK(hipMemcpyAsync(stg + 8, c.d.jgrp, 9 * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    if (c.d.plan.wave_major)
      HIPCHK(hipMemcpyAsync(stg + 48, c.d.woff + wm_waves(c.P), sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    c.timer.mark("layout launches");
    return 0;
  }
  c.timer.mark("layout launches");
  // read back by a kernel into the pinned stage: uv's DMA holds the copy
  // engine (uv itself is taken after the pair lists are enqueued, which do
  // not read it)
  void* stg_d = nullptr;
  HIPCHK(hipHostGetDevicePointer(&stg_d, stg, 0));
  uint8_t* sd = static_cast<uint8_t*>(stg_d);
  HostCopySet cs;
  cs.add(sd, c.poff + c.N, sizeof(int64_t));
  cs.add(sd + 8, c.d.jgrp, 9 * sizeof(int32_t));
  if (c.d.plan.wave_major) cs.add(sd + 48, c.d.woff + wm_waves(c.P), sizeof(int32_t));
  launch_copy_to_host(cs, c.s);
  return 0;
}
int read_pair_total(Setup& c) {
  const uint8_t* stg = c.h->stage;
  HIPCHK(hipStreamSynchronize(c.s));
  std::memcpy(&c.n_pairs, stg, sizeof(int64_t));
  int32_t g[9];
  std::memcpy(g, stg + 8, sizeof(g));
  c.d.xcd_slice_max = 0;
  for (int i = 0; i < 8; ++i) c.d.xcd_slice_max = std::max(c.d.xcd_slice_max, g[i + 1] - g[i]);
  if (c.d.plan.wave_major) {  // the wave-major copy's slot total, and its cap
    int32_t slots = 0;
    std::memcpy(&slots, stg + 48, sizeof(slots));
    c.shape.wm_slots = slots;
    plan_from_shape(c);
    if (!c.d.plan.wave_major) c.d.woff = nullptr;  // (its buffer goes back with the problem's)
  }
  c.timer.mark("layouts (device)");
  return 0;
}

// The Schur pass's shape, the pinned scalar mirror, the pair lists' buffers
// and the wave-major stream's.
int alloc_pair_lists(Setup& c) {
  DevProblem& d = c.d;
  if (c.n_pairs >= int64_t(INT32_MAX)) return fail(SFM_EINVAL, "too many Schur pairs for 32-bit offsets");
  d.n_blk = int64_t(c.C) * (c.C + 1) / 2;
  // the shape follows the mean pair count: the host's estimate on
  // host-counted problems (either layout path, so both choose alike), else
  // the device's count.  The estimate counts every unordered pair of a
  // point's observations, so it undercounts when a camera sees a point twice
  // (a same-camera pair is an ordered pair of the diagonal block); it picks
  // the lanes per block only -- the pair buffer is sized by twice the
  // estimate, an upper bound of the true count either way.
  d.n_pairs = c.plan.host_counts && !c.cam_slice.empty() ? c.pairs_est : c.n_pairs;
  c.shape.n_pairs = d.n_pairs;
  plan_from_shape(c);  // (the shape is complete: the plan is final)
  constexpr size_t kScalHostBytes = sizeof(double) * (kNumScalars + 1 + 17);
  if (c.h->scal_host.reserve(kScalHostBytes, kScalHostBytes, nullptr)) return fail(SFM_ENOMEM, "hipHostMalloc failed");
  d.scal_host = c.h->scal_host;
  c.grp_host = reinterpret_cast<int64_t*>(d.scal_host + kNumScalars + 1);
  c.uv_err_host = reinterpret_cast<int32_t*>(c.grp_host + 16);
  // (and the wave-major stream's, its slot total known by now: filled once
  // uv_pm is, layout_wave_major)
  const bool ok = c.alloc(d.blk, std::max<size_t>(1, size_t(d.n_blk))) &&
                  (c.d.plan.small_setup || c.alloc(d.seg, size_t(d.n_blk) + 1)) &&
                  c.alloc(d.bpts, std::max<size_t>(1, size_t(c.n_pairs))) &&
                  (!c.d.plan.wave_major || (c.alloc(d.uv_wm, 2 * 64 * size_t(c.shape.wm_slots)) && c.alloc(d.cam_wm, 64 * size_t(c.shape.wm_slots))));
  return ok ? 0 : c.rc;
}

void pair_lists_small(Setup& c) {
  DevProblem& d = c.d;
  launch_small_pairs_fill(c.C, d.n_blk, c.d_cam_off, c.cm_order, d.cam_pm, c.pt_s, d.pt_off, d.seg, d.bpts, c.s);
  launch_blk(c.C, d.blk, c.s);
  d.bperm = nullptr;
  d.srec = nullptr;
  d.n_bslots = d.n_blk;
}

int pair_lists_sorted(Setup& c) {
  DevProblem& d = c.d;
  hipStream_t s = c.s;
  const int64_t n_pairs = c.n_pairs;
  uint32_t *bk_a = nullptr, *bk_b = nullptr;
  int32_t* bv = nullptr;
  const int64_t nk = std::max<int64_t>({n_pairs, d.n_blk, 1});
  if (!(c.tmp(bk_a, size_t(nk)) && c.tmp(bk_b, size_t(nk)) && c.tmp(bv, size_t(nk)))) return c.rc;
  const size_t need = std::max(setup_sort_bytes(n_pairs, 32), setup_sort_bytes(d.n_blk, 32));
  if (need > c.sort_bytes) {
    uint8_t* tb = nullptr;
    if (!c.tmp(tb, need)) return c.rc;
    c.sort_tmp = tb;
    c.sort_bytes = need;
  }
  launch_pair_fill(c.N, c.pair_order, d.cam_pm, c.pt_s, d.pt_off, c.poff, c.C, bk_a, bv, s);
  HIPCHK(sort_pairs32(c.sort_tmp, c.sort_bytes, bk_a, bk_b, bv, d.bpts, n_pairs,
                      uint64_t(std::max<int64_t>(1, d.n_blk)) - 1, s));
  launch_seg(d.n_blk, bk_b, n_pairs, d.seg, s);
  launch_blk(c.C, d.blk, s);
  // ---- k_schur_pts work order: XCD-aware (ba_setup.hip k_bperm_*).
  // Block (c1, c2)'s pairs gather records of points camera c1 sees, so a
  // row c1 (its blocks c2 >= c1) reads one camera's ~N/C point records
  // (C3: ~0.5 MB).  Rows go to 8 groups of contiguous rows with equal pair
  // totals; group x's blocks, row by row (descending pair count within a
  // row, so a wave's blocks run lists of nearly equal length), fill
  // workgroups x, x + 8, x + 16, ... -- the ones dealt to one XCD
  // (round-robin placement: a speed assumption only, MI355X_MICROARCH.md),
  // so a row's records stay in that XCD's L2 while its blocks run.  Slots
  // past a group's end hold -1 (an empty list).  Small reduced systems
  // (keyframe-sized solves: everything fits one L2) keep the plain block
  // order (bperm = nullptr).  The group sizes come back with the final
  // synchronisation of set_problem.
  d.bperm = nullptr;
  d.srec = nullptr;
  d.n_bslots = d.n_blk;
  if (d.plan.xcd_block_order) {
    const int per = 64 / d.plan.schur_pts_sub * (kThreads / 64);
    int32_t *sorted = nullptr, *row_x = nullptr;
    int64_t* grp = nullptr;
    if (!(c.tmp(sorted, size_t(d.n_blk)) && c.tmp(row_x, size_t(c.C)) && c.tmp(grp, 16) &&
          c.alloc(d.bperm, size_t(bperm_slots_bound(d.n_blk, per))) &&
          c.alloc(d.srec, size_t(bperm_slots_bound(d.n_blk, per)))))
      return c.rc;
    HIPCHK(launch_bperm(c.C, d.n_blk, n_pairs, d.seg, d.blk, per, bk_a, bk_b, bv, sorted, row_x, grp, c.sort_tmp,
                        c.sort_bytes, d.bperm, d.srec, s));
    HIPCHK(hipMemcpyAsync(c.grp_host, grp, sizeof(int64_t) * 16, hipMemcpyDeviceToHost, s));
    c.bperm_per = per;
  }
  return 0;
}

// Per-iteration arrays and the dense system (the Late route's parameter blob
// among them, and the empty one of a problem without parameters).
int alloc_solver_arrays(Setup& c) {
  sfm_ba_handle* h = c.h;
  DevProblem& d = c.d;
  const size_t C = size_t(c.C), P = size_t(c.P), npad = size_t(d.N_pad);
  d.n = 6 * c.C;
  d.ld = ((d.n + 1 + kNB - 1) / kNB) * kNB;
  d.nblk = d.ld / kNB;
  const ProblemPlan& pp = d.plan;
  d.max_blocks = max_blocks(c.shape, pp, d.xcd_slice_max);
  if (c.plan.route == ParamRoute::Late || c.plan.route == ParamRoute::None)
    if (int rc = alloc_params(c)) return rc;
  // eu: pass A stores u at the camera-major position it runs at (coalesced)
  // and pass B gathers it through pos[]: 85 + 31 -> 60 + 41 us per C3
  // iteration against a point-major scatter, S and steps bitwise equal
  d.ptG = nullptr;
  d.camS = nullptr;
  const size_t tiles = size_t(d.nblk) * d.nblk;
  bool ok = c.alloc(d.cam_new, 6 * C) && c.alloc(d.X_new, 3 * P) && c.alloc(d.scale_c, 6 * C) &&
            c.alloc(d.scale_p, 3 * P) && c.alloc(d.diag_c, 6 * C) && c.alloc(d.diag_p, 3 * P) &&
            c.alloc(d.camR, size_t(kCamR) * C) && c.alloc(d.camRn, 12 * C) &&
            c.alloc(d.eu, size_t(kEU) * npad) && c.alloc(d.ypt, 3 * P) &&
            c.alloc(d.ptV, size_t(kPtV) * P) && c.alloc(d.ptL, size_t(kPtL) * P) &&
            c.alloc(d.ptS, size_t(kPtS) * std::max<size_t>(1, P)) &&
            (!pp.large_system || c.alloc(d.ptG, size_t(kPtG) * std::max<size_t>(1, P))) &&
            (!pp.large_system || c.alloc(d.camS, size_t(kCamSR) * std::max<size_t>(1, C))) &&
            c.alloc(d.Ucam, size_t(kUcam) * C) && c.alloc(d.jpart, 27 * std::max<size_t>(1, npad / 64)) &&
            c.alloc(d.dpart, 27 * std::max<size_t>(1, npad / 64)) && c.alloc(d.S, size_t(d.ld) * d.ld) &&
            (!(sharded(h) || pp.force_pack) || c.alloc(d.Spack, packed_size(d.n))) &&
            c.alloc(d.invL, size_t(d.nblk) * kNB * kNB) && c.alloc(d.flags, size_t(d.nblk)) &&
            c.alloc(d.cflags, 2 * tiles) &&
            c.alloc(d.cticket, 5);  // task ticket, walker-role ticket, back-substitution role ticket, a panel's two
  if (!ok) return c.rc;
  ok = c.alloc(d.ysol, size_t(d.ld)) && c.alloc(d.fail, size_t(1)) &&
       c.alloc(d.partials, size_t(kNumPartialSlots) * d.max_blocks) &&
       c.alloc(d.scal, size_t(kNumScalars) + 1);  // + the Cholesky failure int (k_reduce_batch)
  return ok ? 0 : c.rc;
}

// The wave-major copy of the point-major stream, from uv_pm / cam_pm (on st:
// the stream that made uv_pm).
void layout_wave_major(Setup& c, hipStream_t st) {
  DevProblem& d = c.d;
  if (c.d.plan.wave_major) launch_wm_fill(c.P, d.pt_off, d.woff, d.cam_pm, d.uv_pm, d.cam_wm, d.uv_wm, st);
}

// Deferred uv, by now up or nearly (and before it the parameters): its two
// layouts and its finite check on the side stream, behind its copy and beside
// the pair lists (the index layouts they read are complete: the host
// synchronised on them), the check read back by a kernel with the final
// synchronisation.
int layout_deferred_uv(Setup& c) {
  sfm_ba_handle* h = c.h;
  DevProblem& d = c.d;
  c.worker.join();
  if (c.uv_state.load(std::memory_order_acquire) != 1) return fail(SFM_EIO, "observation upload failed");
  c.timer.mark("uv upload (worker)");
  hipStream_t u = h->ustream;
  launch_uv_layout(c.N, d.N_pad, d.order, d.wcam, d.cam_rng, c.d_cam_off, c.cm_order, c.in_uv, d.uv_pm, d.uv_cm, c.err,
                   u);
  layout_wave_major(c, u);
  void* ue_d = nullptr;
  HIPCHK(hipHostGetDevicePointer(&ue_d, c.uv_err_host, 0));
  HostCopySet cs;
  cs.add(ue_d, c.err + 2, sizeof(int32_t));
  launch_copy_to_host(cs, u);
  HIPCHK(hipEventRecord(h->uev_uv, u));  // (the solve stream waits for it after its own fills, in finish)
  return 0;
}

// What is left of the parameters' way to the device once everything else is
// enqueued.
int finish_params(Setup& c) {
  switch (c.plan.route) {
    case ParamRoute::None:
    case ParamRoute::Early:  // (upload_params_early, before the layouts)
      return 0;
    case ParamRoute::Side:  // enqueued at one of three points; the solve stream takes them here
      if (c.plan.deferred_uv && c.param_state.load(std::memory_order_acquire) != 1)
        return fail(SFM_EIO, "parameter upload failed");
      HIPCHK(hipStreamWaitEvent(c.s, c.h->uev, 0));
      return 0;
    case ParamRoute::Late: {
      // the stage is free: the n_pairs readback synchronised the stream
      if (int rc = stage_reserve(c.h, c.plan.pl_bytes)) return rc;
      fill_param_stage(c, c.h->stage);
      HIPCHK(hipMemcpyAsync(c.d.Kc, c.h->stage, c.plan.pl_bytes, hipMemcpyHostToDevice, c.s));
      return 0;
    }
  }
  return 0;
}

// The last fills, and the end-of-call synchronisation rule.
// Small problems end without a synchronisation: every host-to-device copy
// came from the pinned stage, nothing is read back, so the pair lists and
// uploads run on while the caller enqueues the solve (stream order covers
// every reader; the scratch buffers stay scratch, and the stage is next
// written by a call that synchronises first).  Otherwise: the k_schur_pts
// group sizes come back, copies from pageable host memory (the caller's
// arrays, this call's vectors) complete, and the scratch buffers are retired.
// (SFM_SYNC_SETUP=1: always synchronise, so that a fault in a layout kernel
// is reported by set_problem itself, not by the next call)
int finish(Setup& c) {
  sfm_ba_handle* h = c.h;
  DevProblem& d = c.d;
  hipStream_t s = c.s;
  {
    // the walker stores only the lower 16x16 blocks of each W_k (k_chol_fused)
    Fill32Set fs;
    fs.add(d.S, sizeof(double) * size_t(d.ld) * d.ld, 0);
    fs.add(d.invL, sizeof(double) * size_t(d.nblk) * kNB * kNB, 0);
    fs.add(d.flags, sizeof(int32_t) * size_t(d.nblk), 0);
    fs.add(d.cflags, sizeof(int32_t) * 2 * size_t(d.nblk) * d.nblk, 0);
    fs.add(d.cticket, 5 * sizeof(unsigned long long), 0);
    fs.add(d.partials, sizeof(double) * size_t(kNumPartialSlots) * d.max_blocks, 0);
    launch_fill32(fs, s);
  }
  h->chol_epoch = 0;
  h->bs_epoch = 0;
  d.n_cu = h->n_cu;
  c.timer.mark("pairs + params launches");
  static const bool sync_setup = env_flag("SFM_SYNC_SETUP");
  const bool deferred_uv = c.plan.deferred_uv;
  if (deferred_uv) HIPCHK(hipStreamWaitEvent(s, h->uev_uv, 0));
  if (c.d.plan.small_setup && c.plan.route == ParamRoute::Early && !c.bperm_per && !sync_setup) return 0;
  const DevPool::Drained idle{s};
  if (int rc = hip_rc(SFM_EIO, "hipStreamSynchronize(s)", idle.rc)) return rc;
  if (deferred_uv && *c.uv_err_host != INT32_MAX)
    return fail(SFM_EINVAL, "non-finite observation at " + std::to_string(*c.uv_err_host));
  if (c.bperm_per) {
    int64_t m_max = 1;
    for (int x = 0; x < 8; ++x) m_max = std::max<int64_t>(m_max, (c.grp_host[8 + x] + c.bperm_per - 1) / c.bperm_per);
    d.n_bslots = m_max * 8 * c.bperm_per;
  }
  h->pool.retire_scratch(idle);
  c.timer.mark("pair lists + uploads (device)");
  return 0;
}

int run_setup(Setup& c, const double* K9, const double* rot, const double* t) {
  const hostlayout::SetupPlan& plan = c.plan;
  const bool side = plan.route == ParamRoute::Side;
  int rc = 0;
  if ((rc = open_uploads(c, K9, rot, t))) return rc;
  if ((rc = upload_inputs(c))) return rc;  // (Side, deferred uv: the worker enqueues the parameters too)
  if (!plan.host_counts && (rc = validate_on_device(c))) return rc;
  c.timer.mark("upload + validate");
  if ((rc = report_first_bad_observation(c))) return rc;
  camera_runs(c);
  if ((rc = alloc_layouts(c))) return rc;
  if ((rc = upload_runs_blob(c))) return rc;
  if (plan.route == ParamRoute::Early && (rc = upload_params_early(c))) return rc;
  if (c.d.plan.small_setup) {
    if ((rc = layout_small(c))) return rc;
  } else {
    if ((rc = layout_sorted(c))) return rc;
    if ((rc = enqueue_total_readback(c))) return rc;
    if (side && !plan.deferred_uv) {  // Side, in line: beside the layout kernels, ahead of their round trip
      if ((rc = enqueue_side_params(c))) return rc;
      c.timer.mark("parameter upload (side stream)");
    }
    if ((rc = read_pair_total(c))) return rc;
  }
  if ((rc = alloc_pair_lists(c))) return rc;
  if (c.d.plan.small_setup) pair_lists_small(c);
  else if ((rc = pair_lists_sorted(c))) return rc;
  if ((rc = alloc_solver_arrays(c))) return rc;
  c.h->pool.trim();  // earlier problems' buffers this one did not reuse
  if (plan.deferred_uv && (rc = layout_deferred_uv(c))) return rc;
  if (!plan.deferred_uv) layout_wave_major(c, c.s);
  if (side && c.d.plan.small_setup && (rc = enqueue_side_params(c))) return rc;  // Side, small path: no layout round trip to hide behind
  if ((rc = finish_params(c))) return rc;
  return finish(c);
}

}  // namespace

int sfm_ba_set_problem(sfm_ba_handle* h, int64_t n_obs, const double* obs_uv, const int32_t* cam_idx,
                       const int32_t* pt_idx, int32_t n_cams, const double* K9, const double* rot, const double* t,
                       int32_t n_pts, const double* X) {
  SFM_TRACE("sfm_ba_set_problem");
  if (!h) return fail(SFM_EINVAL, "handle is NULL");
  if (n_obs < 0 || n_cams < 0 || n_pts < 0) return fail(SFM_EINVAL, "negative size");
  if (n_obs > 0 && (!obs_uv || !cam_idx || !pt_idx)) return fail(SFM_EINVAL, "observation arrays are NULL");
  if (n_cams > 0 && (!K9 || !rot || !t)) return fail(SFM_EINVAL, "camera arrays are NULL");
  if (n_pts > 0 && !X) return fail(SFM_EINVAL, "point array is NULL");
  if (n_obs > int64_t(INT32_MAX) - 64 * int64_t(n_cams))
    return fail(SFM_EINVAL, "more than 2^31-1 observations per shard");
  Setup c(h, n_obs, obs_uv, cam_idx, pt_idx, n_cams, n_pts, X);
  HIPCHK(hipSetDevice(h->device));
  const DevPool::Drained idle{h->stream};
  if (int rc = hip_rc(SFM_EIO, "hipStreamSynchronize(h->stream)", idle.rc)) return rc;
  h->drop_problem(idle);
  read_knobs(&h->knobs, kKnobsProblem);
  c.timer.mark("sync + free");
  h->d.C = n_cams;
  h->d.P = n_pts;
  h->d.N = n_obs;
  ProblemGuard guard{c};
  if (int rc = run_setup(c, K9, rot, t)) return rc;
  guard.committed = true;
  h->has_problem = true;
  return 0;
}
