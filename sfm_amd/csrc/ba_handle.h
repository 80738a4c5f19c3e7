// The bundle adjuster's handle and what the files that work on it share:
// ba_solver.hip (the LM loop's drivers, the collectives, the C ABI) and ba_problem.hip
// (sfm_ba_set_problem).  Internal: nothing here is part of include/sfm_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "ba_device.h"
#include "ba_host_layout.h"
#include "dev_mem.h"
#include "../../include/sfm_amd.h"

enum Phase { kPhJac = 0, kPhCamRed, kPhPtEval, kPhPtPrep, kPhSchur, kPhChol, kPhBack, kPhBacksub, kPhOther, kNumPh };

// The distributed factor's panel layout: plain data, assigned afresh by
// dist_prepare whenever the problem, the panel width or the ranks changed.
struct DistLayout {
  int pt = 0, nblk = 0, n = 0, nranks = 0, rank = 0;  // the layout below was made for
  int64_t total = 0;                // doubles of all panel rectangles
  int64_t bcast_cap = 0;            // largest broadcast (doubles)
  std::vector<int64_t> count, poff; // per panel: rectangle doubles, offset in the panel image
};

// The streams first (stream, then those that work beside it): members are
// destroyed in reverse order, so the buffers and events go before them.
struct sfm_ba_handle {
  sfm::Stream stream;
  // set_problem's uploads beside the layout kernels (large problems): the
  // parameters (uev), and uv from a worker thread (uev_uv)
  sfm::Stream ustream;
  sfm::Event uev, uev_uv;
  int device = 0;
  sfm::DevProblem d;
  sfm::PinArr<double> scal_host;  // d.scal_host: the scalars' pinned mirror, kept for the handle's life
  int32_t bs_epoch = 0;          // stamp of the last back-substitution launch (k_backsolve flags)
  int32_t chol_epoch = 0;        // launches of the fused Cholesky since the last set_problem
  // ba_plan.h: the switches (the problem's half read by set_problem, the
  // solve's by each solve) and the running solve's plan; the problem's plan
  // lies with the problem (d.plan)
  sfm::SolveKnobs knobs;
  sfm::SolvePlan plan;
  // multi-GPU
  struct CommDestroy { void operator()(ncclComm_t c) const { ncclCommDestroy(c); } };
  std::unique_ptr<ncclComm, CommDestroy> comm;
  int nranks = 1, rank = 0;
  void set_ranks(int n, int r) { comm.reset(), nranks = n, rank = r; }  // (every way to set the collectives starts here)
  // every buffer d points into, set_problem's scratch, earlier problems' for reuse: keyframe-sized solves
  // (CSfM::bundleAdjustment after every keyframe) allocate nothing; set_problem initialises what it relies on
  sfm::DevPool pool;
  bool has_problem = false;
  // The problem is gone, its buffers free for the next one.
  void drop_problem(const sfm::DevPool::Drained& idle) {
    pool.retire_all(idle);
    d = sfm::DevProblem();
    d.scal_host = scal_host;
    has_problem = false;
  }
  // host-callback collective (sfm_ba_set_host_comm: tests run the sharded
  // path with several ranks on one GPU, where RCCL allows one rank per GPU)
  sfm_allreduce_fn host_fn = nullptr;
  void* host_user = nullptr;
  std::vector<double> host_buf, host_buf2;
  // ... with broadcast and reduce-scatter too (sfm_ba_set_host_collectives);
  // without it the distributed factor builds both from host_fn's all-reduce
  sfm_collective_fn coll_fn = nullptr;
  void* coll_user = nullptr;
  // distributed reduced-camera factor (sfm_ba_set_distributed_factor): 1-D
  // block-cyclic column panels of dist_pt 64-column tiles; 0 = every rank
  // factors the all-reduced system (replicated)
  int dist_pt = 0;
  // ... and what outlives a layout: the collectives' stream, the events, the buffers
  struct DistBufs : DistLayout {
    sfm::Stream cstream;            // RCCL: the collectives' own stream (look-ahead)
    sfm::Event ev_packed, ev_free[2], ev_arrived[2];
    sfm::Event ev_sent;             // the partial panels are packed
    std::vector<sfm::Event> ev_red; // [np] panel k's reduce has landed (owner)
    sfm::DevArr<double> send;       // [total] this rank's partial panels (own ones: zeros)
    sfm::DevArr<double> recv;       // [total] the other ranks' sums of the own panels
    sfm::DevArr<double> bcast;      // [2][bcast_cap]: panel k travels in half k % 2
    sfm::DevArr<int64_t> off_send;  // [np] panel offset in send, -1 for own panels (device)
  } dist;
  // out-of-place target of the collectives enqueued inside a gated phase of
  // the device LM loop (allreduce below); grown on demand
  sfm::DevArr<double> ar_tmp;
  // SFM_EMULATE_IDENTICAL_RANKS=k (tests, read by sfm_ba_set_comm): every sum
  // collective returns k times its one-rank result, i.e. the sum over k
  // ranks holding the same shard, so a one-GPU run sees the stale-buffer
  // hazards of a multi-rank one
  int emulate_ranks = 1;
  // device-driven LM loop: the state block (ba_lm.h; the host driver keeps
  // its own on the stack), its pinned mirror and the trace buffer (grown to
  // the iteration cap)
  sfm::DevArr<sfm::LmCtl> lm_ctl;
  sfm::PinArr<sfm::LmCtl> lm_ctl_host;
  // (pinned host memory: the deciding workgroups write the few entries
  // straight to the host, which reads them after the batch's synchronisation)
  sfm::PinArr<sfm_ba_iteration> lm_trace;
  int lm_trace_cap = 0;
  // one-shot sfm_ba_solve on a small problem: every batch's control readback
  // also brings the parameters (cam | X) into param_host, so the final
  // download needs no further round trip (param_host_valid until consumed)
  bool prefetch_params = false;
  bool param_host_valid = false;
  sfm::PinArr<double> param_host;
  // pinned staging for every host <-> device transfer of set_problem,
  // get_parameters and the LM trace: a pageable copy goes through the
  // runtime's own staging (C1: the 320-KB uv upload took 131 us, the 49-KB
  // parameter download ~100 us), a pinned one is a single DMA.  Grown
  // geometrically, only while the stream is idle.
  sfm::PinArr<uint8_t> stage;
  // device LM loop: the evaluation's k_cam_prep also makes the accepted
  // candidate current (k_lm_accept folded in; its grid covers the copy)
  int accept_grid = 0;  // < 0: done by the deciding reduction (AcceptFold)
  // The step's radius-dependent preparation (point factor, k_obs_prep_rc,
  // diagonal blocks) folded into the evaluation (plan.prep_folded): the
  // radius changes only in the step's decision, so an evaluation prepares
  // the coming step.  eval_radius: that step's radius (host loop; the device
  // loop's kernels read LmCtl::radius).  prep_fresh: the prep on the device
  // is for the current radius; set by the evaluation, cleared when an
  // unsuccessful or invalid step paused the loop (LmCtl::prep_stale, which
  // either driver answers with lm_rearm), after which compute_step runs the
  // stand-alone kernels first.
  double eval_radius = 0.0;
  bool prep_fresh = false;
  // cams_staged: the evaluation's k_cam_sum_diag left the cameras' staged
  // records (plan.stage_cams), so the Schur pair pass skips k_cam_stage_rot --
  // an unsuccessful step leaves the cameras, and with them the records, as
  // they are.
  bool cams_staged = false;
  int n_cu = 0;  // compute units of the device (queried once)
  // profiling
  bool profiling = false;
  std::vector<sfm::Event> ev;
  int ev_used = 0;
  std::vector<std::pair<int, int>> ev_marks;  // (phase, event index of start); end = start + 1
  double phase_ms[kNumPh] = {0};
  int phase_count[kNumPh] = {0};
};

// The pinned staging buffer with room for `bytes` (ba_solver.hip).  Growing it
// frees the old buffer, so nothing may still read or write it: every caller
// has synchronised the stream (set_problem, get_parameters), and a
// keyframe-sized set_problem, which returns with its uploads from the stage
// still in flight, is always followed by a synchronising call before the
// stage is written again.  The rule is checked there: a stream found busy is
// drained first.
int stage_reserve(sfm_ba_handle* h, size_t bytes);
using sfm::kStageMaxBytes;  // transfers above it bypass the stage (ba_host_layout.h)
using sfm::hostlayout::StageLayout;

using sfm::env_flag;  // (ba_plan.h)

// SFM_TIMING=1: host phase times of sfm_ba_set_problem and of the device LM
// loop's batches on stderr.
struct HostTimer {
  bool on = env_flag("SFM_TIMING");
  const char* tag = "set_problem";
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void mark(const char* what) {
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[%s] %-22s %8.3f ms\n", tag, what,
                 std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

inline bool sharded(const sfm_ba_handle* h) { return h->comm != nullptr || h->host_fn != nullptr; }

inline size_t packed_size(int n) { return size_t(n) * (n + 1) / 2 + size_t(n); }
