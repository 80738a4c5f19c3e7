// The Levenberg-Marquardt trust-region bookkeeping of Ceres 1.12
// (TrustRegionMinimizer + LevenbergMarquardtStrategy),
// once: a state block (LmCtl) and three transitions on it, fed by the scalar
// block a phase's reduction leaves.  The device loop runs them in k_lm_* /
// the last workgroup of k_reduce_batch_lm, the host loop calls them between
// its phases (ba_solver.hip: run_device_lm, run_host_lm), and the CPU
// sanitizer program replays the oracle's traces through them
// (tests/asan/asan_main.cpp).  No HIP here: plain C++ for any compiler.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/sfm_amd.h"

#ifdef __HIPCC__
#define SFM_LM_FN __host__ __device__ inline
#else
#define SFM_LM_FN inline
#endif

namespace sfm {

// Index of scalar results (device array `scal`, doubles).
enum Scalar {
  kCost = 0,        // cost at current x (Jacobian pass)
  kGradMaxCam,      // max |g| over camera params
  kGradMaxPt,       // max |g| over point params
  kXNorm2Cam,       // sum x^2 over cameras
  kXNorm2Pt,        // sum x^2 over points
  kModelChange,     // model cost change
  kNewCost,         // cost at the candidate
  kStep2Pt,         // sum dx^2 over points
  kStep2Cam,        // sum dx^2 over cameras
  kBadStep,         // > 0 if the step or candidate is non-finite / V not PD
  kCholFail,        // reserved (the Cholesky flag is an int, fetched separately)
  kBadCam,          // > 0 if the camera step is non-finite
  kBadBack,         // > 0 if the point step is non-finite
  kModelChangePt,   // point share of the model cost change (k_backsub_b; kModelChange holds the observations')
  kNumScalars
};

// LM loop state.  run_step gates compute_step's kernels (0 once done, or
// while paused), run_eval the accept copy and the evaluation (1 after an
// accepted step, until lm_post).  error: bits 2 / 4, a persistent grid's
// hand-off timed out (back substitution / Cholesky); bit 8, the initial cost
// is not finite.  The driver reports them.
struct LmCtl {
  int32_t run_step, run_eval, done, termination, error;
  // The evaluation prepares the coming step (prep_fold, from the driver: SolvePlan::prep_folded).  An
  // unsuccessful or invalid step then pauses the loop (run_step = 0, prep_stale = 1): the radius
  // changed with no evaluation to follow, and the driver, which enqueues the stand-alone prep
  // kernels only when it knows they are needed, re-arms the loop with them in front.
  int32_t prep_fold, prep_stale;
  int32_t iteration, num_consecutive_invalid;
  int32_t n_succ, n_unsucc, n_invalid, n_resid, n_jac, n_lin, trace_len;
  double radius, decrease_factor, cost, grad_max, x_norm;
  sfm_ba_iteration pending;  // an accepted iteration, completed after its evaluation
  int32_t max_iter, max_invalid;
  double ftol, gtol, ptol, max_radius, min_radius, min_rel_dec;
  uint32_t red_count;  // workgroups of k_reduce_batch_lm done (reset by the last)
  double init_cost, init_grad;  // the initial evaluation (lm_init), for the summary
};

// trace_len counts every record, also those past the capacity
SFM_LM_FN void lm_push(LmCtl* c, sfm_ba_iteration* trace, int cap, const sfm_ba_iteration& it) {
  if (c->trace_len < cap) trace[c->trace_len] = it;
  ++c->trace_len;
}
SFM_LM_FN void lm_finish(LmCtl* c, int term) {
  c->termination = term;
  c->done = 1;
  c->run_step = 0;
  c->run_eval = 0;
  c->prep_stale = 0;
}

// after compute_step's reduction (scal: model change, candidate cost, step
// norms, bad-step flags; the Cholesky failure int after the scalars)
SFM_LM_FN void lm_decide(LmCtl* c, const double* scal, sfm_ba_iteration* trace, int cap) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (c->done || !c->run_step) {  // (or paused: the batch's remaining iterations do nothing)
    c->run_eval = 0;
    return;
  }
  ++c->iteration;
  sfm_ba_iteration itr;
  itr.iteration = c->iteration;
  itr.step_is_valid = 0;
  itr.step_is_successful = 0;
  itr.reserved = 0;
  itr.cost = 0.0;
  itr.cost_change = 0.0;
  itr.gradient_max_norm = 0.0;
  itr.step_norm = 0.0;
  itr.relative_decrease = 0.0;
  itr.trust_region_radius = 0.0;
  c->n_lin++;
  const int chol_fail = *reinterpret_cast<const int*>(scal + kNumScalars);
  // The persistent grids' waits are bounded (roles go by start order, so a
  // partly resident grid still progresses); a timeout ends the solve and the
  // driver reports it.
  if (chol_fail & 6) {
    c->error = chol_fail & 6;
    lm_finish(c, SFM_FAILURE);
    return;
  }
  const bool solve_ok = chol_fail == 0 && !(scal[kBadStep] > 0.0) && !(scal[kBadCam] > 0.0) && !(scal[kBadBack] > 0.0);
  const double model_cost_change = scal[kModelChange] + scal[kModelChangePt];
  itr.step_is_valid = (solve_ok && model_cost_change >= 0.0) ? 1 : 0;
  if (!itr.step_is_valid) {
    ++c->num_consecutive_invalid;
    c->n_invalid++;
    if (c->num_consecutive_invalid >= c->max_invalid) {
      itr.cost = c->cost; itr.gradient_max_norm = c->grad_max; itr.trust_region_radius = c->radius;
      lm_push(c, trace, cap, itr);
      lm_finish(c, SFM_FAILURE);
      return;
    }
    itr.cost = c->cost;
    itr.gradient_max_norm = c->grad_max;
  } else {
    c->num_consecutive_invalid = 0;
    double new_cost = scal[kNewCost];
    if (!std::isfinite(new_cost)) new_cost = DBL_MAX;
    c->n_resid++;
    itr.step_norm = std::sqrt(scal[kStep2Cam] + scal[kStep2Pt]);
    const double step_size_tolerance = c->ptol * (c->x_norm + c->ptol);
    if (itr.step_norm <= step_size_tolerance) {
      itr.cost = c->cost; itr.gradient_max_norm = c->grad_max; itr.trust_region_radius = c->radius;
      lm_push(c, trace, cap, itr);
      lm_finish(c, SFM_CONVERGENCE);
      return;
    }
    itr.cost_change = c->cost - new_cost;
    if (std::fabs(itr.cost_change) <= c->ftol * c->cost) {
      itr.cost = c->cost; itr.gradient_max_norm = c->grad_max; itr.trust_region_radius = c->radius;
      lm_push(c, trace, cap, itr);
      lm_finish(c, SFM_CONVERGENCE);
      return;
    }
    itr.relative_decrease = itr.cost_change / model_cost_change;
    itr.step_is_successful = itr.relative_decrease > c->min_rel_dec;
  }
  if (itr.step_is_successful) {
    c->n_succ++;
    const double q = 2.0 * itr.relative_decrease - 1.0;
    double radius = c->radius / std::fmax(1.0 / 3.0, 1.0 - q * q * q);
    c->radius = std::fmin(c->max_radius, radius);
    c->decrease_factor = 2.0;
    c->pending = itr;  // cost, gradient and radius after the evaluation (lm_post)
    c->run_eval = 1;
    return;
  }
  c->n_unsucc++;
  c->radius = c->radius / c->decrease_factor;
  c->decrease_factor *= 2.0;
  c->run_eval = 0;
  if (c->prep_fold) {  // no evaluation follows: the next step redoes its prep for the new radius
    c->prep_stale = 1;
    c->run_step = 0;
  }
  itr.gradient_max_norm = c->grad_max;
  itr.cost = c->cost;
  itr.trust_region_radius = c->radius;
  lm_push(c, trace, cap, itr);
  if (c->radius < c->min_radius) { lm_finish(c, SFM_CONVERGENCE); return; }
  if (c->iteration >= c->max_iter) { lm_finish(c, SFM_NO_CONVERGENCE); return; }
}

// after the accepted step's evaluation (scal: cost, gradient max norms, |x|^2)
SFM_LM_FN void lm_post(LmCtl* c, const double* scal, sfm_ba_iteration* trace, int cap) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (!c->run_eval) return;
  c->run_eval = 0;
  c->n_jac++;
  c->n_resid++;
  const double cost = scal[kCost];
  c->cost = cost;
  if (!std::isfinite(cost)) { lm_finish(c, SFM_FAILURE); return; }
  c->grad_max = std::fmax(scal[kGradMaxCam], scal[kGradMaxPt]);
  c->x_norm = std::sqrt(scal[kXNorm2Cam] + scal[kXNorm2Pt]);
  sfm_ba_iteration itr = c->pending;
  itr.gradient_max_norm = c->grad_max;
  itr.cost = cost;
  itr.trust_region_radius = c->radius;
  lm_push(c, trace, cap, itr);
  if (c->grad_max <= c->gtol) { lm_finish(c, SFM_CONVERGENCE); return; }
  if (c->iteration >= c->max_iter) { lm_finish(c, SFM_NO_CONVERGENCE); return; }
}

// after the initial evaluation (scal: cost, gradient max norms, |x|^2): the
// state the loop starts from, so that the device loop needs no host round
// trip before the first iteration.  Error bit 8: the initial cost is not
// finite.
SFM_LM_FN void lm_init(LmCtl* c, const double* scal) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double cost = scal[kCost];
  c->cost = cost;
  c->init_cost = cost;
  c->grad_max = std::fmax(scal[kGradMaxCam], scal[kGradMaxPt]);
  c->init_grad = c->grad_max;
  c->x_norm = std::sqrt(scal[kXNorm2Cam] + scal[kXNorm2Pt]);
  if (!std::isfinite(cost)) {
    c->error |= 8;
    lm_finish(c, SFM_FAILURE);
  } else if (c->grad_max <= c->gtol) {
    lm_finish(c, SFM_CONVERGENCE);
  } else if (c->max_iter <= 0) {
    lm_finish(c, SFM_NO_CONVERGENCE);
  }
}

}  // namespace sfm
