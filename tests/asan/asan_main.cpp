// CPU sanitizer run (tests/asan/Makefile, `make -C tests/asan asan`): the host
// code of the drop-in and its checker under AddressSanitizer + UBSan, no GPU.
//
// Covered:
//   * sfm_amd/csrc/ba_host_layout.h -- set_problem's host checks and counts,
//     camera runs / chunk table, the small path's slice sizes and the camera-
//     run blob's bound, the small path's size predicate -- on the C1 scene,
//     shuffled duplicates, an empty camera with single-view points, bad
//     indices / non-finite uv, and the empty problem; every output checked
//     against a naive recount; a hub point seen by every camera, by some twice
//     and three times (the pair buffer's bound 2 * pairs_est, the small
//     path's degree limit at 64 / 65 observations); and the
//     plan of set_problem (regimes, parameter routes, the stage's regions)
//     over a grid of sizes around every threshold, with the Schur shape;
//   * sfm_amd/csrc/owner.h -- Buf's growth (no-op below capacity, one release
//     per growth, a failed allocation leaves it empty and the next reserve
//     succeeds, moves free nothing twice) over a malloc / free policy that
//     fails its k-th allocation, and thread_ctx (a failed init caches nothing,
//     one context per thread, destroyed at thread exit: the leak check), and
//     Pool, the bundle adjuster's problem pool: its hand-out rule against a
//     restatement of the hand-kept one over seeded random scripts and at the
//     literal edges, every allocation of a set-up failing in turn, and the
//     order of stream waits and retirements over a large and a keyframe-sized
//     set-up, a failing one and destroy; and RowTable, the map store's
//     tables: seeded random scripts of reserve / write / commit / truncate
//     against a vector per column at the store's column widths, every
//     allocation of a growth failing in turn (the table as it was, the new
//     columns released, the next reserve succeeds), and the order all
//     allocations, copies, drain, swap;
//   * sfm_amd/csrc/ba_lm.h -- the LM trust-region state machine both loop
//     drivers run: the oracle's 18 branch traces replayed through it
//     (tests/golden/lm_replay.txt), and the branches no scene reaches from
//     literal scalars;
//   * include/sfm_ctracker_compat.hpp -- the pointer dedup / packing of
//     bundleAdjustmentStructAndPose (CSfM.cpp:321-341 gather) and its in-place
//     scatter-back, and the matchFeatures overload, with the C ABI answered by
//     the oracle (this binary links no GPU code: sfm_ba_solve /
//     sfm_match_features below are test stubs over oracle/);
//   * oracle/ (test infrastructure): the BA restatement on the same scenes in
//     all three modes, residuals/Jacobians, the matcher, KLT and GFTT.
// Any sanitizer report aborts the run (halt_on_error), so a clean exit with
// "asan: all checks passed" is the result.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "../../include/sfm_amd.h"
#include "../../include/sfm_ctracker_compat.hpp"
#include "../../sfm_amd/csrc/ba_host_layout.h"
#include "../../sfm_amd/csrc/ba_lm.h"
#include "../../sfm_amd/csrc/ba_plan.h"
#include "../../sfm_amd/csrc/owner.h"

// ---- the oracle's C entry points (oracle/*.cpp, linked in) ----
extern "C" {
struct OOptions;
void oracle_default_options(void* o);
int oracle_ba_solve(const void* opts, int mode, int64_t n_obs, const double* obs_uv, const int32_t* cam_idx,
                    const int32_t* pt_idx, int32_t n_cams, const double* K9, double* rot, double* t, int32_t n_pts,
                    double* X, void* summary, void* trace, int32_t trace_cap, int32_t* trace_len);
int oracle_ba_residuals_jacobians(int64_t n_obs, const double* obs_uv, const int32_t* cam_idx,
                                  const int32_t* pt_idx, const double* K9, const double* rot, const double* t,
                                  const double* X, double* res, double* jac);
int oracle_match_features(const double* pts0, const uint8_t* desc0, int32_t n0, const double* pts1,
                          const uint8_t* desc1, int32_t n1, int32_t nbytes, double ratio_test, double min_distance,
                          double max_distance, int32_t* idx0, int32_t* idx1);
void oracle_min_eigen(const uint8_t* img, int32_t w, int32_t h, float* eig);
void oracle_pyr_down(const uint8_t* src, int32_t w, int32_t h, uint8_t* dst);
void oracle_scharr(const uint8_t* src, int32_t w, int32_t h, int16_t* dxy);
// scene generator (sfm_amd/csrc/scene.cpp, plain C++)
int sfm_scene_generate(int32_t n_cams, int32_t n_pts_total, int32_t p_begin, int32_t p_end, int32_t views,
                       uint64_t seed, double pixel_sigma, double pt_sigma, double rot_sigma, double t_sigma,
                       double* K9, double* rot_true, double* t_true, double* X_true, double* rot_init,
                       double* t_init, double* X_init, double* obs_uv, int32_t* cam_idx, int32_t* pt_idx);

// ---- test stubs of the C ABI the compat header calls (oracle-backed) ----
void sfm_ba_default_options(sfm_ba_options* o) { oracle_default_options(o); }
int sfm_ba_solve(const sfm_ba_options* opts, int32_t mode, int64_t n_obs, const double* obs_uv,
                 const int32_t* cam_idx, const int32_t* pt_idx, int32_t n_cams, const double* K9, double* rot,
                 double* t, int32_t n_pts, double* X, sfm_ba_summary* summary, sfm_ba_iteration* trace,
                 int32_t trace_cap, int32_t* trace_len) {
  return oracle_ba_solve(opts, mode, n_obs, obs_uv, cam_idx, pt_idx, n_cams, K9, rot, t, n_pts, X, summary, trace,
                         trace_cap, trace_len);
}
int sfm_match_features(int32_t, const double* pts0, const uint8_t* desc0, int32_t n0, const double* pts1,
                       const uint8_t* desc1, int32_t n1, int32_t desc_bytes, double ratio_test, double min_distance,
                       double max_distance, int32_t* idx0, int32_t* idx1, int32_t* n_matches) {
  const int r = oracle_match_features(pts0, desc0, n0, pts1, desc1, n1, desc_bytes, ratio_test, min_distance,
                                      max_distance, idx0, idx1);
  if (r < 0) return r;
  *n_matches = r;
  return 0;
}
}

static int g_checks = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checks;                                                                  \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

// the environment read_knobs sees in here
static std::map<std::string, std::string> g_env;
static const char* fake_env(const char* name) {
  auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}

struct Scene {
  int C = 0, P = 0;
  std::vector<double> K9, rot, t, X, uv;
  std::vector<int32_t> cam, pt;
  int64_t N() const { return int64_t(cam.size()); }
};

static Scene make_scene(int C, int P, int views, uint64_t seed) {
  Scene s;
  s.C = C;
  s.P = P;
  const int64_t N = int64_t(P) * views;
  s.K9.resize(9 * size_t(C));
  s.rot.resize(3 * size_t(C));
  s.t.resize(3 * size_t(C));
  s.X.resize(3 * size_t(P));
  s.uv.resize(2 * size_t(N));
  s.cam.resize(size_t(N));
  s.pt.resize(size_t(N));
  std::vector<double> rt(3 * size_t(C)), tt(3 * size_t(C)), Xt(3 * size_t(P));
  const int rc = sfm_scene_generate(C, P, 0, P, views, seed, 0.5, 0.01, 1e-3, 0.01, s.K9.data(), rt.data(),
                                    tt.data(), Xt.data(), s.rot.data(), s.t.data(), s.X.data(), s.uv.data(),
                                    s.cam.data(), s.pt.data());
  CHECK(rc == 0);
  return s;
}

// A naive restatement of hostlayout's outputs, for comparison.
static void check_layout(const Scene& s, const char* name) {
  const int C = s.C, P = s.P;
  const int64_t N = s.N();
  std::vector<int32_t> cam_cnt(size_t(C) + 4), pc(size_t(P) + 1);
  std::vector<int32_t> cam_slice;
  int64_t pairs_est = -1;
  sfm::hostlayout::check_and_count(N, s.uv.data(), s.cam.data(), s.pt.data(), C, P, C <= 127, cam_cnt.data(),
                                   pc.data(), &cam_slice, &pairs_est);
  // first bad observation per kind
  int32_t f[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
  for (int64_t i = 0; i < N; ++i) {
    if ((s.cam[i] < 0 || s.cam[i] >= C) && f[0] == INT32_MAX) f[0] = int32_t(i);
    if ((s.pt[i] < 0 || s.pt[i] >= P) && f[1] == INT32_MAX) f[1] = int32_t(i);
    if (!(std::isfinite(s.uv[2 * i]) && std::isfinite(s.uv[2 * i + 1])) && f[2] == INT32_MAX) f[2] = int32_t(i);
  }
  CHECK(cam_cnt[0] == f[0] && cam_cnt[1] == f[1] && cam_cnt[2] == f[2] && cam_cnt[3] == INT32_MAX);
  const bool bad = f[0] != INT32_MAX || f[1] != INT32_MAX || f[2] != INT32_MAX;
  if (bad) {
    std::printf("  %-14s N=%-7lld C=%-4d P=%-6d rejected at observation %d (as the device validation reports)\n",
                name, (long long)N, C, P, std::min({f[0], f[1], f[2]}));
    return;
  }
  std::vector<int32_t> cc(size_t(C), 0), pp(size_t(P) + 1, 0);
  for (int64_t i = 0; i < N; ++i) {
    ++cc[size_t(s.cam[i])];
    ++pp[size_t(s.pt[i])];
  }
  for (int c = 0; c < C; ++c) CHECK(cam_cnt[4 + size_t(c)] == cc[size_t(c)]);
  CHECK(std::equal(pp.begin(), pp.end(), pc.begin()));
  int64_t pe = 0;
  for (int p = 0; p < P; ++p) pe += int64_t(pp[size_t(p)]) * (pp[size_t(p)] - 1) / 2;
  CHECK(pe == pairs_est);
  // camera runs and the chunk table
  sfm::hostlayout::Runs r;
  sfm::hostlayout::camera_runs(C, cam_cnt.data() + 4, &r);
  int64_t np = 0, nch = 0;
  for (int c = 0; c < C; ++c) {
    CHECK(r.cam_off[size_t(c) + 1] - r.cam_off[size_t(c)] == cc[size_t(c)]);
    CHECK(r.cam_rng[2 * size_t(c)] == np && r.cam_rng[2 * size_t(c) + 1] == np + cc[size_t(c)]);
    for (int64_t w = np / 64; w < (np + cc[size_t(c)] + 63) / 64; ++w) CHECK(r.wcam[size_t(w)] == c);
    np += (cc[size_t(c)] + 63) / 64 * 64;
    nch += (cc[size_t(c)] + 63) / 64;
  }
  CHECK(r.npad == np && int64_t(r.chunks.size()) == nch);
  int64_t covered = 0;
  for (const auto& ch : r.chunks) {
    CHECK(ch.cnt >= 1 && ch.cnt <= 64 && ch.pos % 64 == 0);
    CHECK(ch.pos >= r.cam_rng[2 * size_t(ch.cam)] && ch.pos + ch.cnt <= r.cam_rng[2 * size_t(ch.cam) + 1]);
    CHECK(ch.first == r.cam_off[size_t(ch.cam)] + (ch.pos - r.cam_rng[2 * size_t(ch.cam)]));
    covered += ch.cnt;
  }
  CHECK(covered == N);
  // the camera-run blob (cam_rng | wcam | cam_off | chunks | pt_off | fill)
  // within its bound, each part 256-aligned as StageLayout adds it
  auto al = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t blob = al(4 * r.cam_rng.size()) + al(4 * r.wcam.size()) + al(4 * r.cam_off.size()) +
                      al(16 * r.chunks.size()) + al(4 * (size_t(P) + 1)) + al(4 * (size_t(P) + size_t(C)));
  CHECK(blob <= sfm::hostlayout::runs_blob_bound(C, N, P));
  // the small path's size predicate, against its bounds restated: these
  // scenes all fit, except where a camera count is above the plain Schur order
  {
    bool fits = N > 0 && N <= 65536 && C > 0 && C <= 256 && int64_t(C) * (C + 1) / 2 <= 8192 && nch <= 2048;
    for (int p = 0; p < P; ++p) fits = fits && pp[size_t(p)] <= 64;
    CHECK(sfm::hostlayout::small_setup_fits(N, C, P, cam_cnt.data() + 4, pc.data()) == fits);
    CHECK(fits == (N > 0 && C <= 127));
  }
  // small path: slice sizes vs a point-order walk of every camera's run
  if (C <= 127 && P > 0) {
    CHECK(cam_slice.size() == 8 * size_t(C));
    std::vector<std::vector<int32_t>> per(static_cast<size_t>(C));
    std::vector<int64_t> ids(static_cast<size_t>(N));
    std::iota(ids.begin(), ids.end(), 0);
    std::stable_sort(ids.begin(), ids.end(), [&](int64_t a, int64_t b) { return s.pt[a] < s.pt[b]; });
    for (int64_t i : ids) per[size_t(s.cam[i])].push_back(s.pt[i]);
    std::vector<int32_t> jc(8, 0);
    for (int c = 0; c < C; ++c)
      for (size_t k = 0; k < per[size_t(c)].size(); k += 64) ++jc[size_t(int64_t(per[size_t(c)][k]) * 8 / P)];
    CHECK(sfm::hostlayout::small_slice_max(C, cam_cnt.data() + 4, cam_slice) ==
          *std::max_element(jc.begin(), jc.end()));
  }
  std::printf("  %-14s N=%-7lld C=%-4d P=%-6d layout ok (%lld chunks, %lld pairs est.)\n", name, (long long)N, C, P,
              (long long)nch, (long long)pairs_est);
}

// A duplicate-heavy input: point 0 seen once by every one of 60 cameras, then
// again by some of them -- two cameras three times in all (degree 64), and
// with `extra` one more camera twice (degree 65).  The small path sizes the
// pair buffer 2 * pairs_est without a device count, so that must bound the
// pair total by k_pair_count's rule (ba_setup.hip: for each observation, the
// other observations of its point with camera >= its own), which pairs_est
// itself undercounts here; and the hub's degree alone decides the small path.
static void check_duplicate_hub(bool extra) {
  Scene s = make_scene(60, 300, 6, 41);
  {
    Scene e = s;
    e.cam.clear();
    e.pt.clear();
    e.uv.clear();
    auto add = [&](int32_t c, int32_t p, double u, double v) {
      e.cam.push_back(c);
      e.pt.push_back(p);
      e.uv.push_back(u);
      e.uv.push_back(v);
    };
    for (size_t i = 0; i < s.cam.size(); ++i)
      if (s.pt[i] != 0) add(s.cam[i], s.pt[i], s.uv[2 * i], s.uv[2 * i + 1]);
    // (spread through the caller's order: every 25th observation is followed by one of the hub's)
    std::vector<int32_t> hub;
    for (int c = 0; c < s.C; ++c) hub.push_back(c);
    for (int c : {3, 3, 59, 59}) hub.push_back(c);  // cameras 3 and 59 (the last) three times
    if (extra) hub.push_back(20);                   // camera 20 twice
    Scene m = e;
    m.cam.clear();
    m.pt.clear();
    m.uv.clear();
    size_t h = 0;
    for (size_t i = 0; i < e.cam.size(); ++i) {
      m.cam.push_back(e.cam[i]);
      m.pt.push_back(e.pt[i]);
      m.uv.push_back(e.uv[2 * i]);
      m.uv.push_back(e.uv[2 * i + 1]);
      if (i % 25 == 24 && h < hub.size()) {
        m.cam.push_back(hub[hub.size() - 1 - h]);  // the repeats first, cameras descending
        m.pt.push_back(0);
        m.uv.push_back(100.0 + double(h));
        m.uv.push_back(200.0 - double(h));
        ++h;
      }
    }
    CHECK(h == hub.size());
    s = m;
  }
  const int C = s.C, P = s.P;
  const int64_t N = s.N();
  std::vector<int32_t> cam_cnt(size_t(C) + 4), pc(size_t(P) + 1);
  std::vector<int32_t> cam_slice;
  int64_t pairs_est = -1;
  sfm::hostlayout::check_and_count(N, s.uv.data(), s.cam.data(), s.pt.data(), C, P, true, cam_cnt.data(), pc.data(),
                                   &cam_slice, &pairs_est);
  CHECK(cam_cnt[0] == INT32_MAX && cam_cnt[1] == INT32_MAX && cam_cnt[2] == INT32_MAX);
  CHECK(pc[0] == (extra ? 65 : 64));
  CHECK(cam_cnt[4 + 3] >= 3 && cam_cnt[4 + 59] >= 3);
  // k_pair_count's rule, naively
  std::vector<std::vector<int32_t>> cams_of(static_cast<size_t>(P));
  for (int64_t i = 0; i < N; ++i) cams_of[size_t(s.pt[size_t(i)])].push_back(s.cam[size_t(i)]);
  int64_t pairs = 0, est = 0, same = 0;
  for (const auto& v : cams_of) {
    for (size_t a = 0; a < v.size(); ++a)
      for (size_t b = 0; b < v.size(); ++b)
        if (a != b && v[b] >= v[a]) {
          ++pairs;
          same += v[a] == v[b];
        }
    est += int64_t(v.size()) * (int64_t(v.size()) - 1) / 2;
  }
  CHECK(est == pairs_est);
  CHECK(same == (extra ? 14 : 12));     // a camera seen three times: 6 ordered pairs, twice: 2
  CHECK(pairs == pairs_est + same / 2);  // the estimate undercounts by the same-camera pairs
  CHECK(pairs > pairs_est && pairs <= 2 * pairs_est);
  // the hub's degree alone takes the problem off the small path
  CHECK(sfm::hostlayout::small_setup_fits(N, C, P, cam_cnt.data() + 4, pc.data()) == !extra);
  for (int p = 1; p < P; ++p) CHECK(pc[size_t(p)] <= 6);
  std::printf("  %-14s N=%-7lld C=%-4d P=%-6d hub degree %d: %lld pairs (%lld of one camera) <= 2 x %lld est., small path %s\n",
              extra ? "dup-hub-65" : "dup-hub-64", (long long)N, C, P, pc[0], (long long)pairs, (long long)same,
              (long long)pairs_est, extra ? "no" : "yes");
}

// set_problem's host plan (hostlayout::plan_setup): the invariants of the
// stage's regions and of the routes over a grid of sizes around every
// threshold, and rows derived from the expressions the plan replaced.
static void check_plan() {
  using sfm::hostlayout::ParamRoute;
  using sfm::hostlayout::plan_setup;
  const size_t MiB = size_t(1) << 20;
  auto al = [](size_t b) { return (b + 255) / 256 * 256; };
  const int64_t Ns[] = {0, 1, 43648, 43690, 43691, 65536, 65537, 262143, 262144, 2000000};
  const int Cs[] = {0, 1, 127, 128, 256, 257, 2000};
  const int Ps[] = {0, 1, 2000, 21800, 60000, 1000000};
  int n = 0;
  for (int64_t N : Ns)
    for (int C : Cs)
      for (int P : Ps) {
        const auto p = plan_setup(N, C, P, false);
        ++n;
        // the stage's regions in use, in order, disjoint, inside the reserved
        // bytes (the input blob only when it is staged; the camera-run blob
        // has il_bound = 0 without host counts)
        CHECK(p.stage_bytes >= 4 * (size_t(C) + 4));
        if (p.stage_in) CHECK(p.in_bytes <= p.stage_bytes);
        CHECK(p.host_counts ? p.il_base >= p.in_bytes && p.il_base + p.il_bound <= p.stage_bytes
                            : p.il_base == 0 && p.il_bound == 0);
        if (p.route == ParamRoute::Early)
          CHECK(p.pl_base >= p.il_base + p.il_bound && p.pl_base + p.pl_bytes <= p.stage_bytes);
        CHECK(p.il_base % 256 == 0 && p.pl_base % 256 == 0);
        // the blobs' pieces, 256-B aligned; the point counts are part of the
        // input blob up to 65536 observations, staged or not
        CHECK(p.o_uv == 0 && p.o_cam == al(16 * size_t(N)) && p.o_pt == p.o_cam + al(4 * size_t(N)));
        CHECK(p.o_pc == (N <= 65536 ? p.o_pt + al(4 * size_t(N)) : 0));
        CHECK(p.in_bytes == p.o_pt + al(4 * size_t(N)) + (N <= 65536 ? al(4 * (size_t(P) + 1)) : 0));
        CHECK(p.o_K == 0 && p.o_c == al(40 * size_t(C)) && p.o_c0 == p.o_c + al(48 * size_t(C)) &&
              p.o_X == p.o_c0 + al(48 * size_t(C)) && p.o_X0 == p.o_X + al(24 * size_t(P)) &&
              p.pl_bytes == p.o_X0 + al(24 * size_t(P)));
        // exactly one route (an enum), None only without parameters
        CHECK((p.route == ParamRoute::None) == (C == 0 && P == 0));
        if (p.route == ParamRoute::Late) CHECK(p.pl_bytes <= MiB);
        if (p.route == ParamRoute::Side) CHECK(p.pl_bytes > MiB);
        if (p.route == ParamRoute::Early) CHECK(p.host_counts);
        if (p.deferred_uv) CHECK(!p.stage_in && N >= 262144);
        if (p.host_counts) CHECK(N <= 65536 && p.stage_in);
        CHECK(p.stage_in == (p.in_bytes <= MiB));
        CHECK(!plan_setup(N, C, P, true).deferred_uv);
      }
  struct Row {
    int64_t N;
    int C, P;
    bool host_counts, deferred;
    ParamRoute route;
    size_t in_bytes;
  };
  const Row rows[] = {
      {0, 0, 0, true, false, ParamRoute::None, 256},
      {0, 3, 5, true, false, ParamRoute::Early, 256},
      {20000, 20, 2000, true, false, ParamRoute::Early, 488448},
      {43648, 1, 10, true, false, ParamRoute::Early, 1047808},
      {43690, 1, 1, false, false, ParamRoute::Late, 1049088},
      {18000, 130, 3000, true, false, ParamRoute::Early, 444416},
      {30000, 256, 60000, true, false, ParamRoute::Side, 960256},
      {44000, 12, 11000, false, false, ParamRoute::Late, 1100288},
      {66000, 50, 22000, false, false, ParamRoute::Side, 1584384},
      {262143, 50, 20000, false, false, ParamRoute::Late, 6291456},
      {262144, 50, 20000, false, true, ParamRoute::Late, 6291456},
      {264000, 100, 22000, false, true, ParamRoute::Side, 6336000},
      {2000000, 500, 200000, false, true, ParamRoute::Side, 48000000},
  };
  for (const Row& r : rows) {
    const auto p = plan_setup(r.N, r.C, r.P, false);
    CHECK(p.host_counts == r.host_counts && p.deferred_uv == r.deferred && p.route == r.route &&
          p.in_bytes == r.in_bytes);
  }
  CHECK(!plan_setup(262144, 50, 20000, true).deferred_uv);  // SFM_SYNC_UV
  // the Schur shape at the two measured points: C3, a mean of 72 pairs per
  // block; C1, ~460 pairs over 210 blocks
  auto sh = sfm::hostlayout::schur_shape(72 * 125250, 125250, nullptr, nullptr);
  CHECK(sh.pts_sub == 8 && !sh.wg_blocks);
  sh = sfm::hostlayout::schur_shape(460 * 210, 210, nullptr, nullptr);
  CHECK(sh.pts_sub == 64 && sh.wg_blocks);
  sh = sfm::hostlayout::schur_shape(460 * 210, 210, "32", "1");  // the overrides: 64 lanes only take workgroup blocks
  CHECK(sh.pts_sub == 32 && !sh.wg_blocks);
  sh = sfm::hostlayout::schur_shape(460 * 210, 210, "7", "0");
  CHECK(sh.pts_sub == 16 && !sh.wg_blocks);
  CHECK(sfm::hostlayout::schur_shape(0, 0, nullptr, nullptr).pts_sub == 8);
  // the same overrides by way of read_knobs, as the library takes them
  auto shape_with = [](int64_t n_pairs, int64_t n_blk, const char* sub, const char* wg) {
    g_env.clear();
    if (sub) g_env["SFM_SCHUR_PTS_SUB"] = sub;
    if (wg) g_env["SFM_SCHUR_WG"] = wg;
    sfm::SolveKnobs k;
    sfm::read_knobs(&k, sfm::kKnobsProblem, fake_env);
    g_env.clear();
    return sfm::hostlayout::schur_shape(n_pairs, n_blk, k.schur_pts_sub, k.schur_wg);
  };
  sh = shape_with(460 * 210, 210, nullptr, nullptr);
  CHECK(sh.pts_sub == 64 && sh.wg_blocks);
  sh = shape_with(460 * 210, 210, "32", "1");
  CHECK(sh.pts_sub == 32 && !sh.wg_blocks);
  sh = shape_with(460 * 210, 210, "7", "0");
  CHECK(sh.pts_sub == 16 && !sh.wg_blocks);
  // the small path's predicate at its bounds (counts made up: one camera, one point)
  {
    const int32_t one_cam[1] = {65536}, pt64[1] = {64}, pt65[1] = {65};
    CHECK(sfm::hostlayout::small_setup_fits(65536, 1, 1, one_cam, pt64));
    CHECK(!sfm::hostlayout::small_setup_fits(65536, 1, 1, one_cam, pt65));   // a point segment too long
    CHECK(!sfm::hostlayout::small_setup_fits(65537, 1, 1, one_cam, pt64));   // too many observations
    std::vector<int32_t> cams(127, 500);
    CHECK(sfm::hostlayout::small_setup_fits(127 * 500, 127, 1, cams.data(), pt64));
    cams.push_back(500);  // 128 cameras: 8256 blocks, the XCD block order
    CHECK(!sfm::hostlayout::small_setup_fits(128 * 500, 128, 1, cams.data(), pt64));
  }
  std::printf("  plan: %d grid points, %zu literal rows, Schur shape, small-path bounds ok\n", n,
              sizeof(rows) / sizeof(rows[0]));
}

// ---- the ownership templates (sfm_amd/csrc/owner.h) ----
// malloc / free with counters; allocation number fail_at (counted from 1) fails
struct TestMem {
  using Stream = const char*;  // "drained" when non-null
  static int allocs, releases, drains, copies, fail_at;
  static bool trace;                      // log "alloc" / "release" too (the row table's order check)
  static size_t last_bytes;               // of the last successful allocation
  static std::vector<void*> released;     // in order
  static std::vector<std::string> log;    // "drain <stream>" per drain, "copy" per copy; the pool's checks add their own entries
  static int alloc(void** p, size_t bytes) {
    if (++allocs == fail_at) return 7;
    *p = std::malloc(bytes);
    last_bytes = bytes;
    if (trace) log.push_back("alloc");
    return *p ? 0 : 1;
  }
  static void release(void* p) {
    ++releases;
    released.push_back(p);
    if (trace) log.push_back("release");
    std::free(p);
  }
  static int drain(Stream s) {
    ++drains;
    log.push_back(std::string("drain ") + s);
    return 0;
  }
  static int copy(void* dst, const void* src, size_t bytes, Stream) {
    ++copies;
    log.push_back("copy");
    std::memcpy(dst, src, bytes);
    return 0;
  }
  static void reset_counts() {
    allocs = releases = drains = copies = fail_at = 0;
    trace = false;
    released.clear();
    log.clear();
  }
};
int TestMem::allocs = 0, TestMem::releases = 0, TestMem::drains = 0, TestMem::copies = 0, TestMem::fail_at = 0;
bool TestMem::trace = false;
size_t TestMem::last_bytes = 0;
std::vector<void*> TestMem::released;
std::vector<std::string> TestMem::log;

struct TestCtx {
  static int inits, fail_inits, live;
  sfm::Buf<TestMem> buf;
  int key = -1;
  TestCtx() { ++live; }
  ~TestCtx() { --live; }
  int init(int k) {
    ++inits;
    if (fail_inits > 0) return --fail_inits, 5;
    key = k;
    return buf.reserve(64, 64, nullptr);
  }
};
int TestCtx::inits = 0, TestCtx::fail_inits = 0, TestCtx::live = 0;

static void check_owner() {
  using B = sfm::Buf<TestMem>;
  TestMem::reset_counts();
  {
    B b;
    CHECK(b.get() == nullptr && b.bytes() == 0);
    CHECK(b.reserve(0, 0, "s") == 0 && TestMem::allocs == 0);  // nothing needed: nothing made
    CHECK(b.reserve(100, 150, "s") == 0 && b.bytes() == 150 && b.get() != nullptr);
    CHECK(TestMem::allocs == 1 && TestMem::releases == 0 && TestMem::drains == 0);  // (no allocation yet: no drain)
    std::memset(b.get(), 0xAB, 150);
    void* p = b.get();
    CHECK(b.reserve(150, 999, "s") == 0 && b.get() == p && b.bytes() == 150);  // below capacity: untouched
    CHECK(b.reserve(1, 1, nullptr) == 0 && b.get() == p && TestMem::allocs == 1);
    CHECK(b.reserve(151, 300, "s") == 0 && b.bytes() == 300);  // growth: one drain, one release
    CHECK(TestMem::allocs == 2 && TestMem::releases == 1 && TestMem::drains == 1);
    std::memset(b.as<uint8_t>(), 0xCD, 300);
    CHECK(b.reserve(301, 400, nullptr) == 0 && TestMem::drains == 1 && TestMem::releases == 2);  // no stream: no drain
    // a failed allocation: empty and consistent, the error returned; the next reserve succeeds
    TestMem::fail_at = TestMem::allocs + 1;
    CHECK(b.reserve(401, 500, "s") == 7);
    CHECK(b.get() == nullptr && b.bytes() == 0 && TestMem::releases == 3);
    CHECK(b.reserve(10, 20, "s") == 0 && b.bytes() == 20 && TestMem::drains == 2);  // (empty: nothing to drain)
    // moves: the source is left empty, nothing is freed twice
    B c(std::move(b));
    CHECK(b.get() == nullptr && b.bytes() == 0 && c.bytes() == 20 && TestMem::releases == 3);
    B e;
    CHECK(e.reserve(8, 8, nullptr) == 0);
    e = std::move(c);  // releases e's own allocation, takes c's
    CHECK(c.get() == nullptr && c.bytes() == 0 && e.bytes() == 20 && TestMem::releases == 4);
    B& self = e;
    e = std::move(self);
    CHECK(e.bytes() == 20 && TestMem::releases == 4);
    std::vector<B> v(3);
    CHECK(v[2].reserve(5, 5, nullptr) == 0);
    v.resize(40);  // relocates by move
    CHECK(v[2].bytes() == 5);
  }
  CHECK(TestMem::releases == 5 + 1 && TestMem::allocs == TestMem::releases + 1);  // (one allocation failed)
  // thread_ctx
  int rc = -1;
  TestCtx::fail_inits = 2;
  CHECK(sfm::thread_ctx<TestCtx>(3, &rc) == nullptr && rc == 5 && TestCtx::live == 0);  // nothing cached ...
  CHECK(sfm::thread_ctx<TestCtx>(3, &rc) == nullptr && rc == 5 && TestCtx::inits == 2);  // ... so init runs again
  TestCtx* a = sfm::thread_ctx<TestCtx>(3, &rc);
  CHECK(a && rc == 0 && a->key == 3 && TestCtx::inits == 3 && TestCtx::live == 1);
  CHECK(sfm::thread_ctx<TestCtx>(3, &rc) == a && rc == 0 && TestCtx::inits == 3);  // cached
  TestCtx* other_key = sfm::thread_ctx<TestCtx>(4, &rc);
  CHECK(other_key && other_key != a && other_key->key == 4 && TestCtx::live == 2);
  TestCtx* in_thread = nullptr;
  int live_in_thread = 0;
  std::thread t([&] {
    int r = -1;
    in_thread = sfm::thread_ctx<TestCtx>(3, &r);
    CHECK(in_thread && r == 0 && sfm::thread_ctx<TestCtx>(3, &r) == in_thread);
    live_in_thread = TestCtx::live;
  });
  t.join();
  CHECK(in_thread != a && in_thread != other_key && live_in_thread == 3);
  CHECK(TestCtx::live == 2);  // the thread's context went with the thread (its buffer: the leak check)
  CHECK(sfm::thread_ctx<TestCtx>(3, &rc) == a);
  std::printf("  Buf: growth, failed allocation, moves ok; thread_ctx: failed init not cached, per thread ok\n");
}

// ---- the bundle adjuster's problem pool (sfm::Pool, owner.h) ----
// The hand-out rule as the handle kept it by hand before the pool existed
// (dalloc / dalloc_tmp / retire_tmps / free_problem / release_pool over three
// containers), with buffer ids in place of pointers.
struct PoolModel {
  std::vector<std::pair<size_t, int>> allocs, tmps;
  std::multimap<size_t, int> pool;
  int next_id = 0;
  // the buffer handed out; *fresh_bytes: the size of a new allocation, 0 for a reused buffer
  int dalloc(size_t count, size_t elem, bool tmp, size_t* fresh_bytes) {
    if (count == 0) count = 1;
    const size_t bytes = (count * elem + 255) & ~size_t(255);
    auto it = pool.lower_bound(bytes);
    std::pair<size_t, int> a(bytes, -1);
    *fresh_bytes = 0;
    if (it != pool.end() && it->first <= 2 * bytes) {
      a = *it;
      pool.erase(it);
    } else {
      a.second = next_id++;
      *fresh_bytes = bytes;
    }
    (tmp ? tmps : allocs).push_back(a);
    return a.second;
  }
  void retire_tmps() {
    for (auto& a : tmps) pool.insert(a);
    tmps.clear();
  }
  void free_problem() {
    for (auto& a : allocs) pool.insert(a);
    allocs.clear();
    retire_tmps();
  }
  std::vector<int> release_pool() {  // the ids freed, in order
    std::vector<int> ids;
    for (auto& kv : pool) ids.push_back(kv.second);
    pool.clear();
    return ids;
  }
};

using TestPool = sfm::Pool<TestMem>;

// One request of `bytes` (as count elements of 1, 4 or 8 bytes) to both; the
// same buffer must come out.  ptr_of: the model's ids as the pool's pointers.
static void* pool_take_both(TestPool& pool, PoolModel& model, std::vector<void*>& ptr_of, size_t count, int elem,
                            bool scratch) {
  size_t fresh = 0;
  const int id = model.dalloc(count, size_t(elem), scratch, &fresh);
  const int allocs0 = TestMem::allocs;
  void* p = nullptr;
  int rc = -1;
  if (elem == 1) {
    uint8_t* q = nullptr;
    rc = pool.take(&q, count, scratch);
    p = q;
  } else if (elem == 4) {
    int32_t* q = nullptr;
    rc = pool.take(&q, count, scratch);
    p = q;
  } else {
    double* q = nullptr;
    rc = pool.take(&q, count, scratch);
    p = q;
  }
  CHECK(rc == 0 && p != nullptr);
  if (fresh) {
    CHECK(TestMem::allocs == allocs0 + 1 && TestMem::last_bytes == fresh && id == int(ptr_of.size()));
    ptr_of.push_back(p);
  } else {
    CHECK(TestMem::allocs == allocs0 && ptr_of[size_t(id)] == p);
  }
  static_cast<uint8_t*>(p)[0] = static_cast<uint8_t*>(p)[std::max<size_t>(count, 1) * size_t(elem) - 1] = 0x5A;  // (the request fits: ASan checks both ends)
  return p;
}
static void pool_trim_both(TestPool& pool, PoolModel& model, const std::vector<void*>& ptr_of) {
  TestMem::released.clear();
  pool.trim();
  const std::vector<int> ids = model.release_pool();
  CHECK(ids.size() == TestMem::released.size());
  for (size_t k = 0; k < ids.size(); ++k) CHECK(ptr_of[size_t(ids[k])] == TestMem::released[k]);
}

static void check_pool_rule() {
  // ---- seeded random scripts against the model ----
  const size_t bases[] = {0, 1, 100, 256, 1000, 4096, 65536, 300000, size_t(1) << 20, size_t(3) << 20};
  int n_takes = 0, n_reused = 0, n_trims = 0;
  for (uint32_t seed = 0; seed < 3000; ++seed) {
    std::mt19937 rng(seed);
    TestMem::reset_counts();
    {
      TestPool pool;
      PoolModel model;
      std::vector<void*> ptr_of;
      const int steps = 10 + int(rng() % 50);
      // (a script stays with three bases, so that equal sizes and sizes about twice another meet often)
      const size_t b3[3] = {bases[rng() % 10], bases[rng() % 10], bases[rng() % 10]};
      for (int k = 0; k < steps; ++k) {
        const uint32_t op = rng() % 16;
        if (op < 10) {
          // a size at or next to b, 2 b, b / 2: the 2x edge from both sides, in bytes and in 256-byte roundings
          size_t b = b3[rng() % 3];
          const uint32_t shape = rng() % 6;
          if (shape == 1) b *= 2;
          if (shape == 2) b /= 2;
          if (shape == 3) b = 2 * ((b + 255) & ~size_t(255));
          if (shape == 4) b = ((b + 255) & ~size_t(255)) / 2;
          const int64_t nudge[] = {0, 0, 0, 1, -1, 256, -256, 257};
          const int64_t want = int64_t(b) + nudge[rng() % 8];
          const size_t bytes = want < 0 ? 0 : size_t(want);
          const int elem = (rng() % 4 == 0) ? 8 : (rng() % 3 == 0) ? 4 : 1;
          const int allocs0 = TestMem::allocs;
          pool_take_both(pool, model, ptr_of, bytes / size_t(elem), elem, op >= 6);
          ++n_takes;
          n_reused += TestMem::allocs == allocs0;
        } else if (op < 12) {
          pool.retire_scratch(TestPool::Drained{"s"});
          model.retire_tmps();
        } else if (op < 15) {
          pool.retire_all(TestPool::Drained{"s"});
          model.free_problem();
        } else {
          pool_trim_both(pool, model, ptr_of);
          ++n_trims;
        }
      }
    }
    CHECK(TestMem::allocs == TestMem::releases);  // the destructor released the rest, each once (and the leak check)
  }
  CHECK(n_reused > n_takes / 10 && n_reused < n_takes * 9 / 10);  // (both branches are well exercised)
  // ---- the edges, literally ----
  TestMem::reset_counts();
  {
    TestPool pool;
    const TestPool::Drained idle{"s"};
    uint8_t *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
    // a count of 0 is a count of 1: a buffer of 256 bytes
    CHECK(pool.take(&a, 0, false) == 0 && a != nullptr && TestMem::last_bytes == 256 && TestMem::allocs == 1);
    pool.retire_all(idle);
    pool.trim();
    CHECK(TestMem::releases == 1);
    // a free buffer of exactly twice the rounded request is reused, one of 256 bytes more is not
    CHECK(pool.take(&a, 1024, false) == 0 && pool.take(&b, 1280, true) == 0 && TestMem::allocs == 3);
    pool.retire_all(idle);
    CHECK(pool.take(&c, 257, false) == 0 && c == a && TestMem::allocs == 3);  // 257 -> 512, 1024 <= 2 * 512
    pool.retire_all(idle);
    CHECK(pool.take(&c, 256, false) == 0 && c != a && c != b && TestMem::allocs == 4 && TestMem::last_bytes == 256);
    CHECK(pool.take(&d, 513, false) == 0 && d == a);   // 513 -> 768: the smallest that fits, not b
    CHECK(pool.take(&d, 640, false) == 0 && d == b);   // 640 -> 768 again: 1280 <= 1536
    pool.retire_all(idle);
    CHECK(pool.take(&d, 639, false) == 0 && d == a);   // (c's 256 bytes are free too, and too small)
    CHECK(pool.take(&d, 639, false) == 0 && d == b);
    // a reused buffer keeps its true capacity: a (1024) went out for 768 and still serves 1024
    pool.retire_all(idle);
    CHECK(pool.take(&d, 1024, false) == 0 && d == a && TestMem::allocs == 4);
    pool.retire_all(idle);
    pool.trim();
    CHECK(TestMem::releases == 4);
    // two equal free buffers: the one retired first comes out first -- the
    // resident ones before the scratch, each in the order taken
    uint8_t *r0 = nullptr, *r1 = nullptr, *s0 = nullptr, *s1 = nullptr, *o = nullptr;
    CHECK(pool.take(&s0, 4096, true) == 0 && pool.take(&r0, 4096, false) == 0 && pool.take(&s1, 4096, true) == 0 &&
          pool.take(&r1, 4096, false) == 0);
    pool.retire_all(idle);
    for (uint8_t* want : {r0, r1, s0, s1}) CHECK(pool.take(&o, 4000, true) == 0 && o == want);
    pool.retire_scratch(idle);  // all four are scratch now, in that order
    for (uint8_t* want : {r0, r1, s0, s1}) CHECK(pool.take(&o, 4096, false) == 0 && o == want);
    CHECK(TestMem::allocs == 8);
  }
  CHECK(TestMem::allocs == TestMem::releases);
  std::printf("  Pool: 3000 scripts against the hand-kept rule (%d requests, %d reused, %d trims), the edges ok\n", n_takes,
              n_reused, n_trims);
}

// A set_problem-like sequence on the pool, as ba_problem.hip calls it: the
// opening wait and drop, resident and scratch buffers, the trim after the
// solver's arrays, then either the closing wait and the scratch's retirement
// (`sync_end`) or nothing.  `side`: what the failure path waits for beside the
// solve stream.  Stops at the first failed request with its code, as
// run_setup does, and then retires as ProblemGuard does.
static const size_t kSetupSizes[] = {48000, 4000, 320000, 64000, 64000, 1200, 9000, 250000, 16, 700000, 30000, 0};
static const bool kSetupScratch[] = {false, true, true, true, true, false, false, true, false, false, false, false};
static int pool_setup(TestPool& pool, size_t scale, bool sync_end, const char* side, std::vector<uint8_t*>* scratch) {
  const TestPool::Drained idle{"stream"};
  pool.retire_all(idle);
  TestMem::log.push_back("retire all");
  for (int k = 0; k < 12; ++k) {
    uint8_t* p = nullptr;
    const int allocs0 = TestMem::allocs, releases0 = TestMem::releases;
    if (const int rc = pool.take(&p, kSetupSizes[k] * scale, kSetupScratch[k])) {
      CHECK(rc == 7 && p == nullptr && TestMem::allocs == allocs0 + 1 && TestMem::releases == releases0);
      pool.retire_all(TestPool::Drained{"stream", side});
      TestMem::log.push_back("retire all");
      return rc;
    }
    if (kSetupScratch[k] && scratch) scratch->push_back(p);
    TestMem::log.push_back("take");
    if (k == 8) pool.trim();  // (after the solver's arrays; three late requests follow: jrec and the like)
  }
  if (!sync_end) return 0;
  const TestPool::Drained done{"stream"};
  pool.retire_scratch(done);
  TestMem::log.push_back("retire scratch");
  return 0;
}

// In the log, every "retire ..." lies behind a drain of each stream in
// `streams` with no "take" in between: nothing enters the free list while a
// stream that was given work on it since may still run.
static void check_retires_drained(std::initializer_list<const char*> streams) {
  const auto& log = TestMem::log;
  for (size_t k = 0; k < log.size(); ++k) {
    if (log[k].rfind("retire", 0) != 0) continue;
    for (const char* s : streams) {
      bool found = false;
      for (size_t j = k; j-- > 0 && log[j] != "take" && !found;) found = log[j] == std::string("drain ") + s;
      CHECK(found);
    }
  }
}

static void check_pool_failure_and_drains() {
  // ---- every allocation of two set-ups in a row failing in turn ----
  int n_failed = 0;
  for (int k = 1;; ++k) {
    TestMem::reset_counts();
    bool failed = false;
    {
      TestPool pool;
      TestMem::fail_at = k;
      int rc = pool_setup(pool, 1, true, "ustream", nullptr);
      if (!rc) rc = pool_setup(pool, 3, false, "ustream", nullptr);  // (reuses little)
      if (!rc) rc = pool_setup(pool, 2, true, nullptr, nullptr);     // (reuses most)
      failed = rc != 0;
      if (failed) {
        CHECK(rc == 7 && TestMem::allocs == k);
        uint8_t* p = nullptr;  // a later request succeeds, and so does a whole set-up
        CHECK(pool.take(&p, 5000, false) == 0 && p != nullptr);
        CHECK(pool_setup(pool, 1, true, "ustream", nullptr) == 0);
      }
    }
    CHECK(TestMem::releases == TestMem::allocs - (failed ? 1 : 0));  // each released once, the failed one never recorded
    if (!failed) break;
    ++n_failed;
  }
  CHECK(n_failed > 12);  // (the first set-up allocates everything it asks for)
  // ---- the drain rule over the four sequences ----
  // a successful large set-up: the parent synchronises the solve stream at
  // the start of sfm_ba_set_problem and once in finish(), and nowhere else
  TestMem::reset_counts();
  {
    TestPool pool;
    std::vector<uint8_t*> scratch;
    CHECK(pool_setup(pool, 1, true, "ustream", &scratch) == 0);
    CHECK(TestMem::drains == 2);
    check_retires_drained({"stream"});
    uint8_t* p = nullptr;  // the scratch is free again: its first buffer answers a request of its size
    CHECK(pool.take(&p, kSetupSizes[1], false) == 0 && p == scratch[0]);
    // a keyframe-sized one returns without synchronising: one wait, and the
    // scratch is on no free list -- a request of its size is a new allocation
    TestMem::reset_counts();
    scratch.clear();
    CHECK(pool_setup(pool, 1, false, "ustream", &scratch) == 0);
    CHECK(TestMem::drains == 1);
    check_retires_drained({"stream"});
    const int allocs0 = TestMem::allocs;
    CHECK(pool.take(&p, kSetupSizes[2], false) == 0 && TestMem::allocs == allocs0 + 1);
    for (uint8_t* q : scratch) CHECK(p != q);
    // ... until the next set-up's opening wait; this one fails at its second
    // new allocation, after the side stream was given work: both streams are
    // waited for before anything is retired, the solve stream first
    TestMem::log.clear();
    TestMem::drains = 0;
    TestMem::fail_at = TestMem::allocs + 2;
    CHECK(pool_setup(pool, 5, true, "ustream", nullptr) == 7);
    CHECK(TestMem::drains == 3 && TestMem::log[TestMem::log.size() - 3] == "drain stream" &&
          TestMem::log[TestMem::log.size() - 2] == "drain ustream" && TestMem::log.back() == "retire all");
    check_retires_drained({"stream"});
    {
      const std::vector<std::string> all = TestMem::log;  // the failure's own retirement: both streams
      TestMem::log.assign(all.end() - 4, all.end());
      check_retires_drained({"stream", "ustream"});
    }
    // the same where the side stream was never created: it is skipped
    TestMem::log.clear();
    TestMem::drains = 0;
    TestMem::fail_at = TestMem::allocs + 1;
    CHECK(pool_setup(pool, 7, true, nullptr, nullptr) == 7 && TestMem::drains == 2);
    // destroy: the caller's wait for the solve stream, then the destructor
    // releases the resident buffers, the scratch and the free list, each once
    CHECK(pool_setup(pool, 1, false, "ustream", nullptr) == 0);
    TestMem::fail_at = 0;
    TestMem::log.clear();
    const TestPool::Drained at_destroy{"stream"};
    CHECK(TestMem::log.size() == 1 && TestMem::log[0] == "drain stream");
    TestMem::released.clear();
  }
  CHECK(TestMem::log.size() == 1);  // (the destructor waits for nothing itself)
  {
    std::vector<void*> r = TestMem::released;
    std::sort(r.begin(), r.end());
    CHECK(!r.empty() && std::adjacent_find(r.begin(), r.end()) == r.end());
  }
  std::printf("  Pool: %d failing allocations leave it consistent; drains: large set-up 2, keyframe-sized 1, failure both streams, destroy ok\n",
              n_failed);
}

// ---- the map store's row tables (sfm::RowTable, owner.h) ----
// The model: one std::vector of bytes per column, holding the committed rows.
template <int K>
struct TableCheck {
  std::array<size_t, K> width;
  sfm::RowTable<TestMem, K> t;
  std::array<std::vector<uint8_t>, K> model;
  int64_t n = 0, cap = 0;
  uint32_t salt;
  TableCheck(std::array<size_t, K> w, uint32_t seed) : width(w), t(w), salt(seed * 2654435761u) {}

  // the table is the model: n, cap, every committed byte (ASan reads each column to its end)
  void same() const {
    CHECK(t.n() == n && t.cap() == cap);
    for (int c = 0; c < K; ++c) {
      CHECK(model[size_t(c)].size() == size_t(n) * width[size_t(c)]);
      CHECK((cap == 0) == (t.template col<uint8_t>(c) == nullptr));
      if (n) CHECK(std::memcmp(t.template col<uint8_t>(c), model[size_t(c)].data(), model[size_t(c)].size()) == 0);
    }
  }
  int reserve(int64_t rows) {
    const int rc = t.reserve(rows, "s");
    if (!rc && rows > cap) cap = std::max<int64_t>({rows, 2 * cap, 1024});  // the documented rule, in rows
    return rc;
  }
  // k rows past n (each cell one pseudo-random byte, repeated), counted only with `commit`
  void write(int64_t k, bool commit) {
    CHECK(n + k <= cap);
    for (int c = 0; c < K; ++c)
      for (int64_t r = n; r < n + k; ++r) {
        salt = salt * 1664525u + 1013904223u;
        std::memset(t.template col<uint8_t>(c) + size_t(r) * width[size_t(c)], int(salt >> 24), width[size_t(c)]);
      }
    if (!commit) return;
    for (int c = 0; c < K; ++c) {
      const uint8_t* p = t.template col<uint8_t>(c) + size_t(n) * width[size_t(c)];
      model[size_t(c)].insert(model[size_t(c)].end(), p, p + size_t(k) * width[size_t(c)]);
    }
    t.commit(k);
    n += k;
  }
  void truncate(int64_t rows) {
    for (int c = 0; c < K; ++c) model[size_t(c)].resize(size_t(rows) * width[size_t(c)]);
    t.truncate(rows);
    n = rows;
  }
  std::array<void*, K> pointers() const {
    std::array<void*, K> p;
    for (int c = 0; c < K; ++c) p[size_t(c)] = t.template col<void>(c);
    return p;
  }
};

template <int K>
static void check_table_script(std::array<size_t, K> width, uint32_t seed, int* n_growths) {
  std::mt19937 rng(seed);
  TableCheck<K> tc(width, seed);
  tc.same();
  const int steps = 8 + int(rng() % 16);
  for (int k = 0; k < steps; ++k) {
    const uint32_t op = rng() % 8;
    if (op < 3) {  // a reserve at, next to or far from the capacity (also below n: a no-op)
      const int64_t base[] = {0, tc.n, tc.cap, 2 * tc.cap, 1024};
      const int64_t want = std::max<int64_t>(0, base[rng() % 5] + int64_t(rng() % 5) - 2 + (rng() % 8 == 0 ? 700 : 0));
      const int64_t cap0 = tc.cap;
      CHECK(tc.reserve(want) == 0);
      *n_growths += tc.cap != cap0;
    } else if (op < 7) {  // rows written into the room there is, most of them committed
      const int64_t room = tc.cap - tc.n;
      if (room) tc.write(rng() % 4 == 0 ? room : 1 + int64_t(rng() % uint32_t(std::min<int64_t>(room, 600))), rng() % 5 != 0);
    } else if (tc.n) {  // a compaction's end: fewer rows count
      tc.truncate(int64_t(rng() % uint32_t(tc.n + 1)));
    }
    tc.same();
  }
}

// A growth of a K-column table with allocation 1 .. K failing in turn, then
// the order of a successful growth's steps from TestMem's trace.
template <int K>
static void check_table_failures(std::array<size_t, K> width) {
  TestMem::reset_counts();
  {
    TableCheck<K> tc(width, 77);
    CHECK(tc.reserve(1) == 0 && tc.cap == 1024);
    tc.write(1000, true);
    for (int j = 1; j <= K; ++j) {
      const auto before = tc.pointers();
      // (TestMem counts a failed attempt as an allocation: j - 1 of them so far)
      const int balance = TestMem::allocs - (j - 1) - TestMem::releases, allocs = TestMem::allocs;
      const int copies = TestMem::copies, drains = TestMem::drains;
      TestMem::fail_at = TestMem::allocs + j;
      CHECK(tc.reserve(tc.cap + 1) == 7);
      TestMem::fail_at = 0;
      CHECK(tc.pointers() == before);
      tc.same();  // n, cap and contents as they were
      CHECK(TestMem::allocs == allocs + j && TestMem::allocs - j - TestMem::releases == balance);  // j - 1 new columns, released again
      CHECK(TestMem::copies == copies && TestMem::drains == drains);  // nothing was enqueued or waited for
      const int64_t cap0 = tc.cap;
      CHECK(tc.reserve(tc.cap + 1) == 0 && tc.cap == 2 * cap0);        // the next reserve succeeds
      tc.same();
      tc.write(30, true);
    }
    // all allocations, then the copies, then the drain, then the swap (the old columns' release)
    TestMem::log.clear();
    TestMem::trace = true;
    CHECK(tc.reserve(tc.cap + 1) == 0);
    TestMem::trace = false;
    std::vector<std::string> want;
    for (const char* step : {"alloc", "copy"}) want.insert(want.end(), size_t(K), step);
    want.push_back("drain s");
    want.insert(want.end(), size_t(K), "release");
    CHECK(TestMem::log == want);
    tc.same();
    // an empty table with columns: nothing to copy, the drain stays (the old columns may be in use)
    tc.truncate(0);
    TestMem::log.clear();
    TestMem::trace = true;
    CHECK(tc.reserve(tc.cap + 1) == 0);
    TestMem::trace = false;
    want.erase(want.begin() + K, want.begin() + 2 * K);
    CHECK(TestMem::log == want);
    // the first growth: columns only
    TableCheck<K> fresh(width, 78);
    TestMem::log.clear();
    TestMem::trace = true;
    CHECK(fresh.reserve(0) == 0 && TestMem::log.empty());  // nothing needed: nothing made
    CHECK(fresh.reserve(5) == 0 && fresh.cap == 1024);
    TestMem::trace = false;
    CHECK(TestMem::log == std::vector<std::string>(size_t(K), "alloc"));
    fresh.same();
  }
  CHECK(TestMem::allocs - K == TestMem::releases);  // the destructors released every column once (and the leak check)
}

static void check_row_table() {
  int n_growths = 0, n_scripts = 0;
  for (uint32_t seed = 0; seed < 3000; ++seed, ++n_scripts) {
    TestMem::reset_counts();
    const size_t W = size_t(1) << (seed % 7);  // the descriptor table's 8 W bytes, W = 1 .. 64
    switch (seed % 3) {
      case 0: check_table_script<4>({4, 4, 4, 1}, seed, &n_growths); break;       // observations
      case 1: check_table_script<5>({24, 4, 4, 4, 1}, seed, &n_growths); break;   // points
      default: check_table_script<2>({8 * W, 4}, seed, &n_growths); break;         // descriptor rows
    }
    CHECK(TestMem::allocs == TestMem::releases);
  }
  CHECK(n_growths > n_scripts);  // (growth is well exercised)
  check_table_failures<4>({4, 4, 4, 1});
  check_table_failures<5>({24, 4, 4, 4, 1});
  check_table_failures<2>({512, 4});
  std::printf("  RowTable: %d scripts of reserve / write / commit / truncate against a vector per column (%d growths); "
              "each allocation of a growth failing in turn leaves it as it was; allocations, copies, drain, swap in order ok\n",
              n_scripts, n_growths);
}

// ---- the LM trust-region state machine (sfm_amd/csrc/ba_lm.h) ----
using sfm::LmCtl;

static LmCtl lm_ctl(int max_iter, int max_invalid, double ftol, double gtol, double ptol, double radius,
                    double max_radius, double min_radius, double min_rel_dec) {
  LmCtl c;
  std::memset(&c, 0, sizeof(c));
  c.run_step = 1;
  c.radius = radius;
  c.decrease_factor = 2.0;
  c.max_iter = max_iter;
  c.max_invalid = max_invalid;
  c.ftol = ftol;
  c.gtol = gtol;
  c.ptol = ptol;
  c.max_radius = max_radius;
  c.min_radius = min_radius;
  c.min_rel_dec = min_rel_dec;
  return c;
}
// Ceres 1.12's defaults (sfm_ba_default_options)
static LmCtl lm_default(int max_iter = 50) { return lm_ctl(max_iter, 5, 1e-6, 1e-10, 1e-8, 1e4, 1e16, 1e-32, 1e-3); }

// a phase's scalar block: the doubles, then the Cholesky flag (an int)
struct Scal {
  double v[sfm::kNumScalars + 1];
  Scal() { std::memset(v, 0, sizeof(v)); }
  Scal& flag(int f) {
    std::memcpy(v + sfm::kNumScalars, &f, sizeof(int));
    return *this;
  }
  Scal& set(int k, double x) {
    v[k] = x;
    return *this;
  }
};
static Scal eval_scal(double cost, double grad, double xnorm2 = 0.0) {
  return Scal().set(sfm::kCost, cost).set(sfm::kGradMaxCam, grad).set(sfm::kXNorm2Cam, xnorm2);
}
static Scal step_scal(double model_change, double new_cost, double step2) {
  return Scal().set(sfm::kModelChange, model_change).set(sfm::kNewCost, new_cost).set(sfm::kStep2Pt, step2);
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// ---- ba_plan.h: which kernel variant each pass runs ----
// Expected values are written out as the drivers and launchers decided them
// before the plan existed (the predicates of sfm_ba_set_problem,
// evaluate_enqueue, compute_step_enqueue and the launchers), not computed by
// the functions under test.
using sfm::Backsub;
using sfm::CamPass;
using sfm::CamSums;
using sfm::LmDriver;
using sfm::PairPass;
using sfm::PointPass;
using sfm::ProblemPlan;
using sfm::ProblemShape;
using sfm::SolveKnobs;
using sfm::SolvePlan;

// A regular scene's shape: every point in 4 views (fewer cameras: in all),
// ~72 pairs per camera block unless said otherwise, the wave-major stream unpadded.
static ProblemShape plan_shape(int C, int P, bool small_fits = false, int64_t pairs_per_blk = 72) {
  ProblemShape sh;
  const int v = std::min(C, 4);
  sh.C = C;
  sh.P = P;
  sh.N = int64_t(P) * v;
  const int64_t per_cam = C ? (sh.N + C - 1) / C : 0;
  sh.n_jchunks = int(C * ((per_cam + 63) / 64));
  sh.N_pad = 64 * int64_t(sh.n_jchunks);
  sh.host_counts = small_fits;
  sh.small_fits = small_fits && sh.n_blk() <= sfm::kSchurXcdMinBlocks;  // (hostlayout::small_setup_fits' bound)
  sh.n_pairs = pairs_per_blk * sh.n_blk();
  sh.wm_slots = int64_t((P + 63) / 64) * v;
  return sh;
}
static bool same_plan(const ProblemPlan& a, const ProblemPlan& b) {
  return a.small_setup == b.small_setup && a.wave_major == b.wave_major && a.schur_pts_sub == b.schur_pts_sub &&
         a.schur_wg_blocks == b.schur_wg_blocks && a.large_system == b.large_system &&
         a.xcd_block_order == b.xcd_block_order && a.pm_backsub == b.pm_backsub &&
         a.force_pack == b.force_pack && a.schur_wgs == b.schur_wgs &&
         a.jac_blocks == b.jac_blocks && a.jac_blocks_rec == b.jac_blocks_rec;
}
static bool same_plan(const SolvePlan& a, const SolvePlan& b) {
  return a.mode == b.mode && a.cams_var == b.cams_var && a.pts_var == b.pts_var && a.sharded == b.sharded &&
         a.lm == b.lm && a.lm_batch == b.lm_batch && a.prep_folded == b.prep_folded && a.cam_sums == b.cam_sums &&
         a.cam_pass == b.cam_pass && a.point_pass == b.point_pass && a.stage_cams == b.stage_cams &&
         a.pair_pass == b.pair_pass && a.cam_records_used == b.cam_records_used &&
         a.dist_factor == b.dist_factor && a.pack_allreduce == b.pack_allreduce && a.backsub == b.backsub &&
         a.nb_cost == b.nb_cost && a.nb_grad_cam == b.nb_grad_cam && a.nb_cam == b.nb_cam && a.nb_pt == b.nb_pt &&
         a.nb_obs == b.nb_obs && a.nb_back == b.nb_back;
}
// how a solve's collectives are set up
enum Comm { kNoComm, kRccl, kHostCb };
static SolvePlan solve_plan(const ProblemShape& sh, const ProblemPlan& pp, int mode, Comm comm = kNoComm,
                            int dist_pt = 0, const SolveKnobs& k = SolveKnobs(), int32_t xcd_slice_max = 0) {
  return sfm::plan_solve(pp, sfm::SolveShape{sh.C, sh.P, sh.N_pad, xcd_slice_max}, mode, comm != kNoComm,
                         comm == kHostCb, dist_pt, k);
}

static void check_solve_plan() {
  const SolveKnobs k0;
  const int SP = SFM_BA_STRUCT_AND_POSE;
  // ---- the switches: each accepts what its site always did ----
  {
    SolveKnobs k;
    g_env.clear();
    sfm::read_knobs(&k, sfm::kKnobsProblem | sfm::kKnobsSolve, fake_env);
    CHECK(k.small_setup && k.pm_wave_major && k.schur_pts_sub == 0 && k.schur_wg == -1 && k.schur_wgs == 0 &&
          !k.force_pack && k.jac_wg_per_xcd == 0 && !k.eval_split && !k.pe_groups1 &&
          !k.host_lm && !k.lm_unfused && !k.no_accept_fold && k.lm_batch == 0);
    g_env = {{"SFM_SMALL_SETUP", "0"},  {"SFM_PM_WAVE_MAJOR", "00"},  {"SFM_SCHUR_PTS_SUB", "7"},
             {"SFM_SCHUR_WG", "0"},     {"SFM_SCHUR_WGS", "9"},
             {"SFM_FORCE_PACK", "1"},   {"SFM_JAC_WG_PER_XCD", "64"},
             {"SFM_EVAL_SPLIT", "1"},   {"SFM_PE_GROUPS1", "1"},      {"SFM_HOST_LM", "1"},
             {"SFM_LM_UNFUSED", "1"},   {"SFM_NO_ACCEPT_FOLD", "1x"}, {"SFM_LM_BATCH", "100"}};
    sfm::read_knobs(&k, sfm::kKnobsProblem | sfm::kKnobsSolve, fake_env);
    CHECK(!k.small_setup && !k.pm_wave_major && k.schur_pts_sub == 16 && k.schur_wg == 0 && k.schur_wgs == 16 &&
          k.force_pack && k.jac_wg_per_xcd == 64 && k.eval_split && k.pe_groups1 &&
          k.host_lm && k.lm_unfused && k.no_accept_fold && k.lm_batch == 64);
    // "off unless 0" against "on only at 1"; numbers that do not count; the clamps
    g_env = {{"SFM_SMALL_SETUP", "no"}, {"SFM_PM_WAVE_MAJOR", ""},   {"SFM_SCHUR_PTS_SUB", "64"},
             {"SFM_SCHUR_WG", "1"},     {"SFM_SCHUR_WGS", "-5"},
             {"SFM_FORCE_PACK", "2"},   {"SFM_JAC_WG_PER_XCD", "-3"},
             {"SFM_EVAL_SPLIT", "0"},   {"SFM_PE_GROUPS1", "yes"},   {"SFM_HOST_LM", ""},
             {"SFM_LM_UNFUSED", "01"},  {"SFM_NO_ACCEPT_FOLD", "0"}, {"SFM_LM_BATCH", "0"}};
    sfm::read_knobs(&k, sfm::kKnobsProblem | sfm::kKnobsSolve, fake_env);
    CHECK(k.small_setup && k.pm_wave_major && k.schur_pts_sub == 64 && k.schur_wg == 1 && k.schur_wgs == 0 &&
          !k.force_pack && k.jac_wg_per_xcd == 0 && !k.eval_split && !k.pe_groups1 &&
          !k.host_lm && !k.lm_unfused && !k.no_accept_fold && k.lm_batch == 1);
    g_env = {{"SFM_SCHUR_WGS", "1000000"}, {"SFM_HOST_LM", "1"}};
    sfm::read_knobs(&k, sfm::kKnobsProblem, fake_env);  // the problem's half alone
    CHECK(k.schur_wgs == 65536 / 8 * 8 && !k.host_lm && k.schur_pts_sub == 0);
    // the retired switches (the Schur / Cholesky overlap, the point-major u
    // scatter) select nothing any more: the plans of the empty environment
    for (const ProblemShape& sh : {plan_shape(130, 1025), plan_shape(60, 1025)}) {
      SolveKnobs kr;
      g_env = {{"SFM_OVERLAP", "1"}, {"SFM_EU_CM", "0"}};
      sfm::read_knobs(&kr, sfm::kKnobsProblem | sfm::kKnobsSolve, fake_env);
      const ProblemPlan pr = sfm::plan_problem(sh, kr), p0 = sfm::plan_problem(sh, k0);
      CHECK(same_plan(pr, p0));
      CHECK(same_plan(solve_plan(sh, pr, SP, kNoComm, 0, kr), solve_plan(sh, p0, SP)));
    }
    g_env.clear();
  }
  // ---- literal rows ----
  // empty sides: nothing divides by zero, the launchers' size guards do the rest
  {
    ProblemShape sh = plan_shape(0, 10);  // no cameras (so no observations)
    ProblemPlan pp = sfm::plan_problem(sh, k0);
    ProblemPlan e;
    CHECK(same_plan(pp, e));  // all defaults: grids of 8, 8 lanes, nothing large
    SolvePlan s = solve_plan(sh, pp, SP), es;
    es.lm = LmDriver::DeviceFused;  // (AcceptFold needs a camera)
    es.cam_sums = CamSums::SumFinalize;
    es.nb_cost = 8;
    es.nb_back = 8;
    CHECK(same_plan(s, es));
    sh = plan_shape(10, 0);  // no points
    pp = sfm::plan_problem(sh, k0);
    CHECK(same_plan(pp, e));
    s = solve_plan(sh, pp, SP);
    es = SolvePlan();
    es.lm = LmDriver::DeviceFusedAcceptFold;
    es.cam_sums = CamSums::SumFinalize;
    es.nb_cost = 8;
    es.nb_grad_cam = 10;
    CHECK(same_plan(s, es));
    sh = ProblemShape();  // nothing at all, the counts never made
    pp = sfm::plan_problem(sh, k0);
    CHECK(same_plan(pp, e));
    CHECK(sfm::max_blocks(sh, pp, 0) == 8);
  }
  // C = 64 / 65: the camera sums leave the point pass, the step's prep folds
  {
    ProblemShape sh = plan_shape(64, 1025);
    ProblemPlan pp = sfm::plan_problem(sh, k0);
    ProblemPlan e;
    e.wave_major = true;
    e.jac_blocks = e.jac_blocks_rec = 32;  // 128 chunks: (128 / 8 + 3) / 4 = 4 workgroups per XCD
    CHECK(same_plan(pp, e));
    SolvePlan s = solve_plan(sh, pp, SP), es;
    es.lm = LmDriver::DeviceFusedAcceptFold;
    es.cam_sums = CamSums::InPointPass;
    es.point_pass = PointPass::Lds64;
    es.nb_cost = 32;
    es.nb_grad_cam = 64;
    es.nb_pt = 5;
    es.nb_obs = 32;  // 128 chunks, no slice sizes: ((128 + 3) / 4 + 7) / 8 = 4 per XCD
    es.nb_back = 8;
    CHECK(same_plan(s, es));
    sh = plan_shape(65, 1025);
    pp = sfm::plan_problem(sh, k0);
    e.jac_blocks = e.jac_blocks_rec = 16;  // 65 chunks: (65 / 8 + 3) / 4 = 2
    CHECK(same_plan(pp, e));
    s = solve_plan(sh, pp, SP);
    es.prep_folded = true;
    es.cam_sums = CamSums::SumDiag;
    es.cam_pass = CamPass::JacObsPrep;
    es.point_pass = PointPass::Lds512x2;
    es.nb_cost = 16;
    es.nb_grad_cam = 65;
    es.nb_obs = 24;  // ((65 + 3) / 4 + 7) / 8 = 3
    CHECK(same_plan(s, es));
    CHECK(es.pair_pass == PairPass::Pts && !es.stage_cams && es.backsub == Backsub::ThreePass);
  }
  // C = 127 / 128: 8128 / 8256 camera blocks against kSchurXcdMinBlocks = 8192
  {
    ProblemShape sh = plan_shape(127, 1025);
    ProblemPlan pp = sfm::plan_problem(sh, k0);
    ProblemPlan e;
    e.wave_major = true;
    e.jac_blocks = e.jac_blocks_rec = 32;  // 127 chunks: (127 / 8 + 3) / 4 = 4
    CHECK(same_plan(pp, e));               // not large: no ptG / camS, no bperm / srec, three-pass backsub
    SolvePlan s = solve_plan(sh, pp, SP), es;
    es.lm = LmDriver::DeviceFusedAcceptFold;
    es.prep_folded = true;
    es.cam_sums = CamSums::SumDiag;
    es.cam_pass = CamPass::JacObsPrep;
    es.point_pass = PointPass::Lds512x2;
    es.pair_pass = PairPass::Pts;
    es.backsub = Backsub::ThreePass;
    es.nb_cost = 32;
    es.nb_grad_cam = 127;
    es.nb_pt = 5;
    es.nb_obs = 32;  // ((127 + 3) / 4 + 7) / 8 = 4
    es.nb_back = 8;
    CHECK(same_plan(s, es));
    sh = plan_shape(128, 1025);
    pp = sfm::plan_problem(sh, k0);
    e.large_system = e.xcd_block_order = e.pm_backsub = true;  // ptG, camS, bperm, srec wanted
    CHECK(same_plan(pp, e));                                   // (128 chunks: 4 workgroups per XCD again)
    s = solve_plan(sh, pp, SP);
    es.stage_cams = es.cam_records_used = true;
    es.pair_pass = PairPass::RotPersistent;
    es.backsub = Backsub::OnePass;
    es.nb_grad_cam = 128;
    es.nb_obs = es.nb_back = 5;  // the one pass: per 256 points
    CHECK(same_plan(s, es));
    // ... which the small setup path never takes (hostlayout::small_setup_fits):
    // the same plans where the host counted the observations
    sh = plan_shape(128, 1025, true);
    pp = sfm::plan_problem(sh, k0);
    CHECK(same_plan(pp, e));
    CHECK(same_plan(solve_plan(sh, pp, SP), es));
  }
  // the accept fold's edge: C <= 256 and 3 P <= 24576
  {
    ProblemPlan e;
    e.wave_major = e.large_system = e.xcd_block_order = e.pm_backsub = true;
    SolvePlan es;
    es.prep_folded = es.stage_cams = es.cam_records_used = true;
    es.cam_sums = CamSums::SumDiag;
    es.cam_pass = CamPass::JacObsPrep;
    es.point_pass = PointPass::Lds512x2;
    es.pair_pass = PairPass::RotPersistent;
    es.backsub = Backsub::OnePass;
    struct Row {
      int C, P, jac, nb_cam, nb_pt;  // jac: 8 (n_jchunks / 8 + 3) / 4 with n_jchunks = 512, 514, 768, 514
      LmDriver lm;
    };
    const Row rows[] = {{256, 8192, 128, 1, 32, LmDriver::DeviceFusedAcceptFold},
                        {257, 8192, 128, 2, 32, LmDriver::DeviceFused},
                        {256, 8193, 192, 1, 33, LmDriver::DeviceFused},
                        {257, 8193, 128, 2, 33, LmDriver::DeviceFused}};
    for (const Row& r : rows) {
      const ProblemShape sh = plan_shape(r.C, r.P);
      const ProblemPlan pp = sfm::plan_problem(sh, k0);
      e.jac_blocks = e.jac_blocks_rec = r.jac;  // (the record-writing grid's cap is 128 per XCD: not reached)
      CHECK(same_plan(pp, e));
      es.lm = r.lm;
      es.nb_cost = r.jac;
      es.nb_grad_cam = r.C;
      es.nb_cam = r.nb_cam;
      es.nb_pt = es.nb_obs = es.nb_back = r.nb_pt;
      CHECK(same_plan(solve_plan(sh, pp, SP), es));
    }
  }
  // C = 512 / 513: the cameras leave the LDS of the point pass and of k_backsub_pm
  {
    ProblemShape sh = plan_shape(512, 8193);
    ProblemPlan pp = sfm::plan_problem(sh, k0);
    ProblemPlan e;
    e.wave_major = e.large_system = e.xcd_block_order = e.pm_backsub = true;
    e.jac_blocks = e.jac_blocks_rec = 256;  // 1024 chunks: (1024 / 8 + 3) / 4 = 32
    CHECK(same_plan(pp, e));
    SolvePlan s = solve_plan(sh, pp, SP), es;
    es.lm = LmDriver::DeviceFused;
    es.prep_folded = es.stage_cams = es.cam_records_used = true;
    es.cam_sums = CamSums::SumDiag;
    es.cam_pass = CamPass::JacObsPrep;
    es.point_pass = PointPass::Lds512x2;
    es.pair_pass = PairPass::RotPersistent;
    es.backsub = Backsub::OnePass;
    es.nb_cost = 256;
    es.nb_grad_cam = 512;
    es.nb_cam = 2;
    es.nb_pt = es.nb_obs = es.nb_back = 33;
    CHECK(same_plan(s, es));
    sh = plan_shape(513, 8193);
    pp = sfm::plan_problem(sh, k0);
    e.pm_backsub = false;
    e.jac_blocks = e.jac_blocks_rec = 128;  // 513 chunks: (513 / 8 + 3) / 4 = 16
    CHECK(same_plan(pp, e));
    s = solve_plan(sh, pp, SP);
    es.point_pass = PointPass::Rc;
    es.backsub = Backsub::ThreePass;
    es.nb_cost = 128;
    es.nb_grad_cam = 513;
    es.nb_cam = 3;
    es.nb_obs = 136;  // no slice sizes: ((513 + 3) / 4 + 7) / 8 = 17 per XCD
    es.nb_back = 40;  // 1025 points per slice: 5 blocks of 256
    CHECK(same_plan(s, es));
    // the observation passes' grid from the largest point slice's chunks, as
    // every problem with observations has them: (70 + 3) / 4 = 18 per XCD
    s = solve_plan(sh, pp, SP, kNoComm, 0, k0, 70);
    es.nb_obs = 144;
    CHECK(same_plan(s, es));
    CHECK(sfm::max_blocks(sh, pp, 0) == 513 && sfm::max_blocks(sh, pp, 70) == 513);  // cameras
    CHECK(sfm::max_blocks(sh, pp, 2100) == 4200);                                    // one slice with most chunks
  }
  // a workgroup per block beyond 64 cameras: the prep does not fold (the pass
  // takes the diagonal blocks itself)
  {
    const ProblemShape sh = plan_shape(70, 1025, false, 460);
    const ProblemPlan pp = sfm::plan_problem(sh, k0);
    ProblemPlan e;
    e.wave_major = true;
    e.schur_pts_sub = 64;                   // 8 -> 64 while below 460 / 10
    e.jac_blocks = e.jac_blocks_rec = 16;   // 70 chunks: (70 / 8 + 3) / 4 = 2
    CHECK(same_plan(pp, e));                // 2485 blocks: above the 1024 of the shape's own choice
    SolveKnobs k;
    k.schur_wg = 1;
    const ProblemPlan pw = sfm::plan_problem(sh, k);
    e.schur_wg_blocks = true;
    CHECK(same_plan(pw, e));
    SolvePlan es;
    es.lm = LmDriver::DeviceFusedAcceptFold;
    es.cam_sums = CamSums::SumFinalize;
    es.cam_pass = CamPass::Jacobian;
    es.point_pass = PointPass::Lds512x2;
    es.pair_pass = PairPass::WgBlocks;
    es.backsub = Backsub::ThreePass;
    es.nb_cost = 16;
    es.nb_grad_cam = 70;
    es.nb_pt = 5;
    es.nb_obs = 24;  // ((70 + 3) / 4 + 7) / 8 = 3
    es.nb_back = 8;
    CHECK(same_plan(solve_plan(sh, pw, SP), es));
  }
  // the three modes, the collectives and every switch alone at C = 130, P = 1025
  const ProblemShape sh130 = plan_shape(130, 1025);
  const ProblemPlan pp130 = sfm::plan_problem(sh130, k0);
  ProblemPlan ep;
  ep.wave_major = ep.large_system = ep.xcd_block_order = ep.pm_backsub = true;
  ep.jac_blocks = ep.jac_blocks_rec = 32;  // 130 chunks: (130 / 8 + 3) / 4 = 4
  CHECK(same_plan(pp130, ep));
  CHECK(sfm::max_blocks(sh130, pp130, 0) == 130);  // cameras; the observation passes' 40 and N_pad / 256 = 33 below
  SolvePlan e130;
  e130.lm = LmDriver::DeviceFusedAcceptFold;
  e130.prep_folded = true;
  e130.cam_sums = CamSums::SumDiag;
  e130.cam_pass = CamPass::JacObsPrep;
  e130.point_pass = PointPass::Lds512x2;
  e130.stage_cams = true;
  e130.pair_pass = PairPass::RotPersistent;
  e130.cam_records_used = true;
  e130.backsub = Backsub::OnePass;
  e130.nb_cost = 32;
  e130.nb_grad_cam = 130;
  e130.nb_pt = e130.nb_obs = e130.nb_back = 5;
  CHECK(same_plan(solve_plan(sh130, pp130, SP), e130));
  {
    SolvePlan e = e130;  // POSE_ONLY: points constant; nothing folds or fuses, three passes
    e.mode = SFM_BA_POSE_ONLY;
    e.pts_var = false;
    e.prep_folded = e.stage_cams = false;
    e.cam_sums = CamSums::SumFinalize;
    e.cam_pass = CamPass::Jacobian;
    e.backsub = Backsub::ThreePass;
    e.nb_obs = 40;  // ((130 + 3) / 4 + 7) / 8 = 5 per XCD
    e.nb_back = 8;
    CHECK(same_plan(solve_plan(sh130, pp130, SFM_BA_POSE_ONLY), e));
    e.mode = SFM_BA_STRUCT_ONLY;  // cameras constant
    e.pts_var = true;
    e.cams_var = false;
    e.cam_sums = CamSums::None;
    e.nb_grad_cam = 1;
    CHECK(same_plan(solve_plan(sh130, pp130, SFM_BA_STRUCT_ONLY), e));
  }
  {
    // sharded: a collective between the camera sums and their use, and between
    // a phase's reduction and the bookkeeping
    SolveKnobs ko;
    const ProblemPlan ps = sfm::plan_problem(sh130, ko);
    CHECK(same_plan(ps, ep));
    SolvePlan e = e130;
    e.sharded = e.pack_allreduce = true;
    e.lm = LmDriver::Device;
    e.prep_folded = e.stage_cams = false;
    e.cam_sums = CamSums::ReduceAllreduceFinalize;
    e.cam_pass = CamPass::Jacobian;
    e.nb_grad_cam = 1;
    CHECK(same_plan(solve_plan(sh130, ps, SP, kRccl, 0, ko), e));
    e.lm = LmDriver::Host;
    CHECK(same_plan(solve_plan(sh130, ps, SP, kHostCb, 0, ko), e));
    e.dist_factor = true;
    CHECK(same_plan(solve_plan(sh130, ps, SP, kHostCb, 2, ko), e));
    CHECK(same_plan(solve_plan(sh130, ps, SP, kRccl, 2, ko), e));
    e = e130;  // a panel width without a communicator changes nothing
    CHECK(same_plan(solve_plan(sh130, pp130, SP, kNoComm, 2), e));
  }
  {
    // the problem's switches, one at a time
    SolveKnobs k = k0;
    k.small_setup = false;  // (not a small-path problem)
    CHECK(same_plan(sfm::plan_problem(sh130, k), ep));
    const ProblemShape sm = plan_shape(20, 1025, true, 460);  // ... and one that is
    CHECK(sfm::plan_problem(sm, k0).small_setup && !sfm::plan_problem(sm, k0).wave_major);
    CHECK(!sfm::plan_problem(sm, k).small_setup && sfm::plan_problem(sm, k).wave_major);
    CHECK(sfm::plan_problem(sm, k0).schur_wg_blocks);  // 210 blocks of 460 pairs
    ProblemPlan e = ep;
    k = k0, k.pm_wave_major = false, e.wave_major = false;
    CHECK(same_plan(sfm::plan_problem(sh130, k), e));
    e = ep, k = k0, k.schur_pts_sub = 32, e.schur_pts_sub = 32;
    CHECK(same_plan(sfm::plan_problem(sh130, k), e));
    e = ep, k = k0, k.schur_wg = 1;  // (only 64 lanes take workgroup blocks)
    CHECK(same_plan(sfm::plan_problem(sh130, k), e));
    e = ep, k = k0, k.schur_wgs = 16, e.schur_wgs = 16;
    CHECK(same_plan(sfm::plan_problem(sh130, k), e));
    e = ep, k = k0, k.jac_wg_per_xcd = 2, e.jac_blocks = 16;
    CHECK(same_plan(sfm::plan_problem(sh130, k), e));
    SolvePlan es = e130;
    es.nb_cost = 16;
    CHECK(same_plan(solve_plan(sh130, sfm::plan_problem(sh130, k), SP), es));
    e = ep, k = k0, k.force_pack = true, e.force_pack = true;
    es = e130, es.pack_allreduce = true;
    CHECK(same_plan(sfm::plan_problem(sh130, k), e));
    CHECK(same_plan(solve_plan(sh130, e, SP), es));
    // the wave-major stream's cap, once its slots are counted
    ProblemShape pad = sh130;
    pad.wm_slots = -1;
    CHECK(sfm::plan_problem(pad, k0).wave_major);  // wanted until then
    pad.wm_slots = (3 * pad.N + 128 * 17) / 128;
    CHECK(sfm::plan_problem(pad, k0).wave_major);
    pad.wm_slots += 1;
    CHECK(!sfm::plan_problem(pad, k0).wave_major);
  }
  {
    // the solve's switches, one at a time
    SolveKnobs k = k0;
    SolvePlan e = e130;
    k.eval_split = true, e.cam_pass = CamPass::Jacobian, e.stage_cams = false;
    CHECK(same_plan(solve_plan(sh130, pp130, SP, kNoComm, 0, k), e));
    e = e130, k = k0, k.pe_groups1 = true, e.point_pass = PointPass::Lds512;
    CHECK(same_plan(solve_plan(sh130, pp130, SP, kNoComm, 0, k), e));
    e = e130, k = k0, k.host_lm = true, e.lm = LmDriver::Host;
    CHECK(same_plan(solve_plan(sh130, pp130, SP, kNoComm, 0, k), e));
    e = e130, k = k0, k.lm_unfused = true, e.lm = LmDriver::Device;
    CHECK(same_plan(solve_plan(sh130, pp130, SP, kNoComm, 0, k), e));
    e = e130, k = k0, k.no_accept_fold = true, e.lm = LmDriver::DeviceFused;
    CHECK(same_plan(solve_plan(sh130, pp130, SP, kNoComm, 0, k), e));
    e = e130, k = k0, k.lm_batch = 5, e.lm_batch = 5;
    CHECK(same_plan(solve_plan(sh130, pp130, SP, kNoComm, 0, k), e));
  }
  // ---- invariants over a grid ----
  std::vector<SolveKnobs> knobs(1, k0);
  auto with = [&](auto set) { knobs.push_back(k0); set(knobs.back()); };
  with([](SolveKnobs& k) { k.small_setup = false; });
  with([](SolveKnobs& k) { k.pm_wave_major = false; });
  for (int sub : {8, 16, 32, 64}) with([sub](SolveKnobs& k) { k.schur_pts_sub = sub; });
  for (int wg : {0, 1}) with([wg](SolveKnobs& k) { k.schur_wg = wg; });
  with([](SolveKnobs& k) { k.schur_pts_sub = 64, k.schur_wg = 1; });  // (the pair that forces workgroup blocks)
  with([](SolveKnobs& k) { k.schur_wgs = 16; });
  with([](SolveKnobs& k) { k.force_pack = true; });
  with([](SolveKnobs& k) { k.jac_wg_per_xcd = 1; });
  with([](SolveKnobs& k) { k.jac_wg_per_xcd = 1000; });
  with([](SolveKnobs& k) { k.eval_split = true; });
  with([](SolveKnobs& k) { k.pe_groups1 = true; });
  with([](SolveKnobs& k) { k.host_lm = true; });
  with([](SolveKnobs& k) { k.lm_unfused = true; });
  with([](SolveKnobs& k) { k.no_accept_fold = true; });
  with([](SolveKnobs& k) { k.lm_batch = 64; });
  int n_plans = 0;
  for (int C : {0, 1, 64, 65, 127, 128, 256, 257, 512, 513, 2000})
    for (int P : {0, 1, 255, 8192, 8193})
      for (int small = 0; small < 2; ++small)
        for (const SolveKnobs& k : knobs) {
          const ProblemShape sh = plan_shape(C, P, small != 0, C <= 64 ? 460 : 72);
          for (Comm comm : {kNoComm, kRccl, kHostCb}) {
            const ProblemPlan pp = sfm::plan_problem(sh, k);
            CHECK(pp.schur_pts_sub == 8 || pp.schur_pts_sub == 16 || pp.schur_pts_sub == 32 || pp.schur_pts_sub == 64);
            CHECK(!pp.schur_wg_blocks || pp.schur_pts_sub == 64);
            CHECK(!pp.xcd_block_order || pp.large_system);
            CHECK(!pp.pm_backsub || pp.large_system);
            CHECK(!(pp.wave_major && pp.small_setup));
            CHECK(pp.jac_blocks >= 8 && pp.jac_blocks % 8 == 0 && pp.jac_blocks_rec >= 8 && pp.jac_blocks_rec % 8 == 0);
            // the largest point slice's chunks: not counted (0), or an eighth of them and ~5% (what
            // sfm_ba_set_problem hands to both)
            const int32_t n_chunks = int32_t(sh.N_pad / 64);
            for (int v = 0; v < 6; ++v) {
              const int mode = v % 3;
              const int32_t slice_max = v < 3 ? 0 : n_chunks / 8 + n_chunks / 128 + 1;
              const int cap = sfm::max_blocks(sh, pp, slice_max);
              const SolvePlan s = solve_plan(sh, pp, mode, comm, 0, k, slice_max);
              ++n_plans;
              const bool fused = s.cam_pass == CamPass::JacObsPrep;
              CHECK(!fused || s.prep_folded);
              CHECK(!s.prep_folded || s.cam_sums == CamSums::SumDiag);
              CHECK((s.cam_sums == CamSums::SumDiag) == s.prep_folded);
              CHECK(!s.prep_folded || (mode == SFM_BA_STRUCT_AND_POSE && !s.sharded));
              CHECK(s.pair_pass != PairPass::RotPersistent || s.cam_records_used);
              CHECK(!s.cam_records_used || pp.large_system);
              CHECK(!s.stage_cams || fused);
              CHECK(s.backsub != Backsub::OnePass || pp.pm_backsub);
              CHECK(s.backsub != Backsub::OnePass || mode == SFM_BA_STRUCT_AND_POSE);
              CHECK(!s.fused_lm() || !s.sharded);
              CHECK(comm != kHostCb || s.lm == LmDriver::Host);
              CHECK((s.cam_sums == CamSums::None) == !s.cams_var);
              for (int nb : {s.nb_cost, s.nb_grad_cam, s.nb_cam, s.nb_pt, s.nb_obs, s.nb_back})
                CHECK(nb >= 1 && nb <= cap);
            }
          }
        }
  std::printf("  solve plan: switches, literal rows, %d plans on the grid ok\n", n_plans);
}

// The oracle's traces of every branch case (tests/golden/lm_replay.txt, from
// lm_branches.json by make_lm_replay.py) replayed through lm_init / lm_decide
// / lm_post: each phase's scalars are rebuilt from the record the phase led
// to, and the state machine must write the oracle's records and counters.
static void check_lm_replay() {
  std::FILE* f = std::fopen("../golden/lm_replay.txt", "r");
  CHECK(f != nullptr);
  int n_cases = 0;
  CHECK(std::fscanf(f, "%d", &n_cases) == 1);
  CHECK(n_cases == 18);
  double worst_radius = 0.0;
  for (int k = 0; k < n_cases; ++k) {
    char name[64];
    int n = 0, max_iter = 0, max_invalid = 0, sm[8];
    double o[7];
    CHECK(std::fscanf(f, " case %63s %d", name, &n) == 2 && n >= 1);
    CHECK(std::fscanf(f, "%d %d %lf %lf %lf %lf %lf %lf %lf", &max_iter, &max_invalid, &o[0], &o[1], &o[2], &o[3], &o[4],
                      &o[5], &o[6]) == 9);
    for (int& s : sm) CHECK(std::fscanf(f, "%d", &s) == 1);
    std::vector<sfm_ba_iteration> rec(static_cast<size_t>(n));
    for (auto& r : rec) {
      r.reserved = 0;
      CHECK(std::fscanf(f, "%d %d %d %lf %lf %lf %lf %lf %lf", &r.iteration, &r.step_is_valid, &r.step_is_successful,
                        &r.cost, &r.cost_change, &r.gradient_max_norm, &r.step_norm, &r.relative_decrease,
                        &r.trust_region_radius) == 9);
    }
    const double ptol = o[2];
    LmCtl c = lm_ctl(max_iter, max_invalid, o[0], o[1], ptol, o[3], o[4], o[5], o[6]);
    // |x| is not in the trace: 0, except at the evaluation before a final
    // record that stopped at the parameter tolerance, where |x| makes that
    // record's step the tolerance
    const sfm_ba_iteration& fin = rec.back();
    const bool ptol_stop = n > 1 && fin.step_is_valid && !fin.step_is_successful && fin.cost_change == 0.0 && fin.step_norm > 0.0;
    int last_eval = 0;
    for (int i = 0; i < n - 1; ++i)
      if (rec[size_t(i)].step_is_successful) last_eval = i;
    auto xnorm2 = [&](int i) {
      const double q = fin.step_norm / ptol;
      return ptol_stop && i == last_eval ? q * q : 0.0;
    };
    std::vector<sfm_ba_iteration> out(size_t(std::max(1, max_iter + 1)));
    const int cap = int(out.size());
    lm_init(&c, eval_scal(rec[0].cost, rec[0].gradient_max_norm, xnorm2(0)).v);
    CHECK(same_bits(c.init_cost, rec[0].cost) && same_bits(c.init_grad, rec[0].gradient_max_norm));
    CHECK(same_bits(c.radius, rec[0].trust_region_radius));
    for (int i = 1; i < n; ++i) {
      CHECK(!c.done);
      const sfm_ba_iteration& r = rec[size_t(i)];
      Scal s = step_scal(r.relative_decrease != 0.0 ? r.cost_change / r.relative_decrease : 1.0, c.cost - r.cost_change,
                         r.step_norm * r.step_norm);
      if (!r.step_is_valid) s.flag(1);
      lm_decide(&c, s.v, out.data(), cap);
      CHECK(c.run_eval == r.step_is_successful);
      if (c.run_eval) lm_post(&c, eval_scal(r.cost, r.gradient_max_norm, xnorm2(i)).v, out.data(), cap);
    }
    CHECK(c.done && c.error == 0);
    CHECK(c.trace_len == n - 1);
    for (int i = 1; i < n; ++i) {
      const sfm_ba_iteration &a = out[size_t(i - 1)], &b = rec[size_t(i)];
      CHECK(a.iteration == b.iteration && a.step_is_valid == b.step_is_valid && a.step_is_successful == b.step_is_successful);
      CHECK(same_bits(a.cost, b.cost) && same_bits(a.cost_change, b.cost_change));
      CHECK(same_bits(a.gradient_max_norm, b.gradient_max_norm) && same_bits(a.step_norm, b.step_norm));
      CHECK(same_bits(a.relative_decrease, b.relative_decrease));
      // (the model change is a quotient of the record's rounded numbers, so rho is the fixture's only to rounding)
      const double d = std::fabs(a.trust_region_radius - b.trust_region_radius) / b.trust_region_radius;
      worst_radius = std::max(worst_radius, d);
      CHECK(d <= 1e-15);
    }
    // the summary the drivers make of the state (+ the initial evaluation)
    const int got[8] = {c.termination, c.iteration, c.n_succ, c.n_unsucc, c.n_invalid, 1 + c.n_resid, 1 + c.n_jac, c.n_lin};
    for (int j = 0; j < 8; ++j) CHECK(got[j] == sm[j]);
  }
  std::fclose(f);
  std::printf("  replay: %d oracle traces reproduced (largest radius difference %.1e relative)\n", n_cases, worst_radius);
}

// The branches the scenes cannot reach, from literal scalars; the expected
// values follow from Ceres 1.12's rules and default options (radius 1e4,
// halved then quartered ... on rejection; radius / max(1/3, 1 - (2 rho - 1)^3)
// on acceptance; 5 consecutive invalid steps fail).
static void check_lm_branches() {
  sfm_ba_iteration tr[8];
  auto started = [&](int max_iter = 50) {
    LmCtl c = lm_default(max_iter);
    lm_init(&c, eval_scal(100.0, 5.0).v);
    CHECK(!c.done && c.run_step == 1 && c.cost == 100.0 && c.grad_max == 5.0 && c.x_norm == 0.0 && c.trace_len == 0);
    return c;
  };
  const Scal accept = step_scal(50.0, 50.0, 1.0);   // rho = (100 - 50) / 50 = 1
  const Scal reject = step_scal(50.0, 150.0, 1.0);  // rho = -1
  const double grown = 1e4 / (1.0 / 3.0);           // rho = 1: 1 - (2 rho - 1)^3 = 0 < 1/3
  // hand-off timeouts (bits 2 and 4 of the Cholesky flag): recorded, FAILURE, no record
  for (int bits : {2, 4, 6}) {
    LmCtl c = started();
    lm_decide(&c, Scal(accept).flag(bits).v, tr, 8);
    CHECK(c.error == bits && c.done && c.termination == SFM_FAILURE && c.trace_len == 0);
    CHECK(c.run_step == 0 && c.run_eval == 0 && c.iteration == 1 && c.n_lin == 1 && c.n_invalid == 0);
  }
  // a non-finite candidate cost counts as DBL_MAX: a valid step, rejected
  for (double bad : {double(NAN), double(INFINITY), -double(INFINITY)}) {
    LmCtl c = started();
    lm_decide(&c, step_scal(50.0, bad, 1.0).v, tr, 8);
    CHECK(!c.done && c.run_eval == 0 && c.run_step == 1 && c.trace_len == 1 && c.n_resid == 1 && c.n_unsucc == 1);
    CHECK(tr[0].step_is_valid == 1 && tr[0].step_is_successful == 0 && tr[0].cost_change == 100.0 - DBL_MAX);
    CHECK(tr[0].relative_decrease == (100.0 - DBL_MAX) / 50.0 && tr[0].cost == 100.0 && tr[0].step_norm == 1.0);
    CHECK(tr[0].trust_region_radius == 5e3 && c.radius == 5e3 && c.decrease_factor == 4.0);
  }
  // an accepted step, its record completed by the evaluation ...
  {
    LmCtl c = started();
    lm_decide(&c, accept.v, tr, 8);
    CHECK(!c.done && c.run_eval == 1 && c.run_step == 1 && c.prep_stale == 0 && c.trace_len == 0 && c.n_succ == 1);
    CHECK(c.radius == grown && c.decrease_factor == 2.0);
    lm_post(&c, eval_scal(50.0, 4.0, 9.0).v, tr, 8);
    CHECK(!c.done && c.run_eval == 0 && c.trace_len == 1 && c.n_jac == 1 && c.n_resid == 2 && c.x_norm == 3.0);
    CHECK(tr[0].iteration == 1 && tr[0].step_is_valid == 1 && tr[0].step_is_successful == 1 && tr[0].cost == 50.0);
    CHECK(tr[0].cost_change == 50.0 && tr[0].relative_decrease == 1.0 && tr[0].gradient_max_norm == 4.0);
    CHECK(tr[0].trust_region_radius == grown);
    // ... and lm_post without an accepted step in flight is a no-op
    const LmCtl before = c;
    lm_post(&c, eval_scal(1.0, 1.0).v, tr, 8);
    CHECK(std::memcmp(&c, &before, sizeof(c)) == 0);
  }
  // a non-finite cost after an accepted step: FAILURE, no record
  {
    LmCtl c = started();
    lm_decide(&c, accept.v, tr, 8);
    lm_post(&c, eval_scal(NAN, 4.0).v, tr, 8);
    CHECK(c.done && c.termination == SFM_FAILURE && c.error == 0 && c.trace_len == 0 && c.n_jac == 1 && c.n_resid == 2);
    CHECK(std::isnan(c.cost) && c.iteration == 1);
  }
  // a non-finite initial cost: error bit 8
  {
    LmCtl c = lm_default();
    lm_init(&c, eval_scal(INFINITY, 5.0).v);
    CHECK(c.done && c.error == 8 && c.termination == SFM_FAILURE && c.init_cost == INFINITY && c.run_step == 0);
  }
  // no iterations allowed; a gradient tolerance met at once comes first
  {
    LmCtl c = lm_default(0);
    lm_init(&c, eval_scal(100.0, 5.0).v);
    CHECK(c.done && c.termination == SFM_NO_CONVERGENCE && c.iteration == 0 && c.error == 0 && c.n_lin == 0);
    c = lm_default(0);
    lm_init(&c, eval_scal(100.0, 1e-10).v);
    CHECK(c.done && c.termination == SFM_CONVERGENCE && c.iteration == 0);
  }
  // the iteration cap reached by an accepted step (after its evaluation) and by a rejected one
  {
    LmCtl c = started(1);
    lm_decide(&c, accept.v, tr, 8);
    CHECK(!c.done && c.run_eval == 1);
    lm_post(&c, eval_scal(50.0, 4.0).v, tr, 8);
    CHECK(c.done && c.termination == SFM_NO_CONVERGENCE && c.trace_len == 1 && c.iteration == 1 && c.cost == 50.0);
    c = started(1);
    lm_decide(&c, reject.v, tr, 8);
    CHECK(c.done && c.termination == SFM_NO_CONVERGENCE && c.trace_len == 1 && c.iteration == 1 && c.run_eval == 0);
    CHECK(tr[0].step_is_successful == 0 && tr[0].relative_decrease == -1.0 && tr[0].trust_region_radius == 5e3);
  }
  // the radius clamp
  {
    LmCtl c = lm_ctl(50, 5, 1e-6, 1e-10, 1e-8, 1e4, 2e4, 1e-32, 1e-3);
    lm_init(&c, eval_scal(100.0, 5.0).v);
    lm_decide(&c, accept.v, tr, 8);
    CHECK(c.radius == 2e4 && grown > 2e4);
  }
  // invalid steps: a negative model change, a failed Cholesky, each bad-step
  // flag; the fifth in a row fails, its record with the radius unchanged
  {
    const Scal invalid[5] = {step_scal(-1.0, 50.0, 1.0), Scal(accept).flag(1), Scal(accept).set(sfm::kBadStep, 1.0),
                             Scal(accept).set(sfm::kBadCam, 1.0), Scal(accept).set(sfm::kBadBack, 1.0)};
    for (const Scal& s : invalid) {
      LmCtl c = started();
      lm_decide(&c, s.v, tr, 8);
      CHECK(!c.done && c.run_eval == 0 && c.n_invalid == 1 && c.num_consecutive_invalid == 1 && c.n_unsucc == 1);
      CHECK(c.n_resid == 0 && c.trace_len == 1 && tr[0].step_is_valid == 0 && tr[0].step_is_successful == 0);
      CHECK(tr[0].cost == 100.0 && tr[0].cost_change == 0.0 && tr[0].step_norm == 0.0 && tr[0].trust_region_radius == 5e3);
      lm_decide(&c, accept.v, tr, 8);  // a valid step resets the run
      CHECK(c.num_consecutive_invalid == 0 && c.run_eval == 1);
    }
    LmCtl c = started();
    for (const Scal& s : invalid) lm_decide(&c, s.v, tr, 8);
    CHECK(c.done && c.termination == SFM_FAILURE && c.n_invalid == 5 && c.n_unsucc == 4 && c.trace_len == 5);
    CHECK(c.radius == 1e4 / 2 / 4 / 8 / 16 && tr[4].trust_region_radius == c.radius && tr[3].trust_region_radius == c.radius);
  }
  // the evaluation prepares the step (prep_fold): a rejected or invalid step
  // pauses the loop for the driver to re-arm, an accepted one does not; a call
  // while paused, or done, only clears run_eval
  for (const Scal& s : {reject, step_scal(-1.0, 50.0, 1.0)}) {
    LmCtl c = started();
    c.prep_fold = 1;
    lm_decide(&c, s.v, tr, 8);
    CHECK(!c.done && c.run_step == 0 && c.prep_stale == 1 && c.run_eval == 0 && c.trace_len == 1);
    LmCtl paused = c;
    c.run_eval = 1;
    lm_decide(&c, accept.v, tr, 8);
    CHECK(std::memcmp(&c, &paused, sizeof(c)) == 0);
  }
  {
    LmCtl c = started();
    c.prep_fold = 1;
    lm_decide(&c, accept.v, tr, 8);
    CHECK(c.run_step == 1 && c.prep_stale == 0 && c.run_eval == 1);
    c = started(1);
    c.prep_fold = 1;
    lm_decide(&c, reject.v, tr, 8);  // the last iteration: done, not paused
    CHECK(c.done && c.prep_stale == 0 && c.run_step == 0);
    LmCtl done = c;
    c.run_eval = 1;
    lm_decide(&c, accept.v, tr, 8);
    CHECK(std::memcmp(&c, &done, sizeof(c)) == 0);
  }
  // a trace of one record: the count goes on, the writes do not
  {
    std::vector<sfm_ba_iteration> one(1);
    LmCtl c = started();
    lm_decide(&c, reject.v, one.data(), 1);
    lm_decide(&c, reject.v, one.data(), 1);
    lm_decide(&c, accept.v, one.data(), 1);
    lm_post(&c, eval_scal(50.0, 4.0).v, one.data(), 1);
    CHECK(c.trace_len == 3 && one[0].iteration == 1 && one[0].trust_region_radius == 5e3 && c.iteration == 3);
  }
  std::printf("  branches: timeouts, non-finite costs, iteration cap, clamp, invalid steps, pause, trace cap ok\n");
}

struct Pt2 {
  double x, y;
};
struct M33 {
  double val[9];
};
struct Desc {
  int rows, cols;
  const uint8_t* data;
};

// compat: gather through aliased per-observation pointers, solve (oracle),
// scatter back; compare with the oracle on the packed arrays directly
static void check_compat(const Scene& s, int mode) {
  const int64_t N = s.N();
  std::vector<double> Xw(s.X), rw(s.rot), tw(s.t);
  std::vector<Pt2> obs(static_cast<size_t>(N));
  std::vector<int> camIdx(static_cast<size_t>(N));
  std::vector<double*> pts(static_cast<size_t>(N)), R(size_t(s.C)), T(size_t(s.C));
  std::vector<M33> K(size_t(s.C));
  for (int64_t i = 0; i < N; ++i) {
    obs[size_t(i)] = Pt2{s.uv[2 * i], s.uv[2 * i + 1]};
    camIdx[size_t(i)] = s.cam[size_t(i)];
    pts[size_t(i)] = &Xw[3 * size_t(s.pt[size_t(i)])];
  }
  for (int c = 0; c < s.C; ++c) {
    R[size_t(c)] = &rw[3 * size_t(c)];
    T[size_t(c)] = &tw[3 * size_t(c)];
    std::memcpy(K[size_t(c)].val, &s.K9[9 * size_t(c)], sizeof(double) * 9);
  }
  sfm_ba_summary sm{};
  const int rc = sfm_compat::bundleAdjustmentStructAndPose(obs, camIdx, K, R, T, pts, mode, nullptr, &sm);
  CHECK(rc == 0);
  // the same solve on the caller's own arrays
  std::vector<double> Xo(s.X), ro(s.rot), to(s.t);
  sfm_ba_options o;
  sfm_ba_default_options(&o);
  sfm_ba_summary so{};
  CHECK(sfm_ba_solve(&o, mode, N, s.uv.data(), s.cam.data(), s.pt.data(), s.C, s.K9.data(), ro.data(), to.data(),
                     s.P, Xo.data(), &so, nullptr, 0, nullptr) == 0);
  // the compat layer renumbers points in first-seen order, which changes the
  // Schur summation order: the same solve up to rounding
  CHECK(so.num_iterations == sm.num_iterations && so.termination_type == sm.termination_type);
  CHECK(std::fabs(so.final_cost - sm.final_cost) <= 1e-9 * std::max(1.0, so.final_cost));
  auto close = [](double a, double b) { return std::fabs(a - b) <= 1e-6 * std::max(1.0, std::fabs(b)); };
  for (int64_t i = 0; i < N; ++i)
    for (int k = 0; k < 3; ++k) CHECK(close(pts[size_t(i)][k], Xo[3 * size_t(s.pt[size_t(i)]) + k]));
  for (size_t k = 0; k < rw.size(); ++k) CHECK(close(rw[k], ro[k]) && close(tw[k], to[k]));
  // unobserved points are never written (no pointer reaches them)
}

int main() {
  std::printf("asan: host layout (ba_host_layout.h)\n");
  Scene c1 = make_scene(20, 2000, 10, 0x5F3D2017ull + 1);  // C1: 20 cams / 2000 points / 20000 obs
  check_layout(c1, "C1");
  Scene dup = make_scene(12, 400, 4, 23);  // shuffled caller order with duplicates
  {
    std::mt19937_64 g(7);
    for (int k = 0; k < 40; ++k) {
      const size_t i = size_t(g() % dup.cam.size());
      dup.cam.push_back(dup.cam[i]);
      dup.pt.push_back(dup.pt[i]);
      dup.uv.push_back(dup.uv[2 * i] + 0.1);
      dup.uv.push_back(dup.uv[2 * i + 1] - 0.1);
    }
    std::vector<size_t> perm(dup.cam.size());
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), g);
    Scene sh = dup;
    for (size_t i = 0; i < perm.size(); ++i) {
      sh.cam[i] = dup.cam[perm[i]];
      sh.pt[i] = dup.pt[perm[i]];
      sh.uv[2 * i] = dup.uv[2 * perm[i]];
      sh.uv[2 * i + 1] = dup.uv[2 * perm[i] + 1];
    }
    dup = sh;
  }
  check_layout(dup, "dup-shuffled");
  Scene emp = make_scene(40, 3000, 6, 31);  // an empty camera and single-view points
  {
    Scene e = emp;
    e.cam.clear();
    e.pt.clear();
    e.uv.clear();
    std::vector<int> seen(size_t(e.P), 0);
    for (size_t i = 0; i < emp.cam.size(); ++i) {
      if (emp.cam[i] == 17) continue;                        // camera 17 sees nothing
      if (emp.pt[i] % 50 == 0 && seen[size_t(emp.pt[i])]++) continue;  // every 50th point: one view
      e.cam.push_back(emp.cam[i]);
      e.pt.push_back(emp.pt[i]);
      e.uv.push_back(emp.uv[2 * i]);
      e.uv.push_back(emp.uv[2 * i + 1]);
    }
    emp = e;
  }
  check_layout(emp, "empty-camera");
  Scene badc = c1;
  badc.cam[777] = badc.C;
  check_layout(badc, "bad-camera");
  Scene badp = c1;
  badp.pt[123] = -1;
  badp.cam[5000] = -3;
  check_layout(badp, "bad-point");
  Scene nanuv = c1;
  nanuv.uv[2 * 999 + 1] = std::nan("");
  nanuv.uv[2 * 4000] = INFINITY;
  check_layout(nanuv, "non-finite-uv");
  Scene none;
  none.C = 3;
  none.P = 0;
  none.K9.assign(27, 0.0);
  check_layout(none, "empty");
  Scene big = make_scene(130, 500, 8, 99);  // above the small path's 127 cameras: no slices
  check_layout(big, "C>127");
  check_duplicate_hub(false);
  check_duplicate_hub(true);

  std::printf("asan: set_problem's host plan (ba_host_layout.h)\n");
  check_plan();
  check_solve_plan();

  std::printf("asan: ownership templates (owner.h)\n");
  check_owner();
  check_pool_rule();
  check_pool_failure_and_drains();
  check_row_table();

  std::printf("asan: LM trust-region state machine (ba_lm.h)\n");
  check_lm_replay();
  check_lm_branches();

  std::printf("asan: compat header over the oracle (gather, solve, scatter-back)\n");
  for (int mode = 0; mode < 3; ++mode) {
    check_compat(c1, mode);
    check_compat(dup, mode);
    check_compat(emp, mode);
    std::printf("  mode %d: C1, dup-shuffled, empty-camera ok\n", mode);
  }
  {
    std::vector<double> res(2 * size_t(c1.N())), jac(18 * size_t(c1.N()));
    CHECK(oracle_ba_residuals_jacobians(c1.N(), c1.uv.data(), c1.cam.data(), c1.pt.data(), c1.K9.data(),
                                        c1.rot.data(), c1.t.data(), c1.X.data(), res.data(), jac.data()) == 0);
    for (double v : res) CHECK(std::isfinite(v));
  }

  std::printf("asan: matcher (compat overload over the oracle), KLT / GFTT oracle kernels\n");
  {
    std::mt19937_64 g(11);
    const int n0 = 500, n1 = 520;
    std::vector<uint8_t> d0(64 * size_t(n0)), d1(64 * size_t(n1));
    for (auto& b : d0) b = uint8_t(g());
    for (auto& b : d1) b = uint8_t(g());
    for (int i = 0; i < n0; ++i) std::memcpy(&d1[64 * size_t(i)], &d0[64 * size_t(i)], 64), d1[64 * size_t(i)] ^= 1;
    std::vector<Pt2> p0(static_cast<size_t>(n0)), p1(static_cast<size_t>(n1));
    std::uniform_real_distribution<double> U(0, 1280), D(-5, 5);
    for (int i = 0; i < n0; ++i) p0[size_t(i)] = Pt2{U(g), U(g) * 0.5625};
    for (int i = 0; i < n1; ++i) p1[size_t(i)] = i < n0 ? Pt2{p0[size_t(i)].x + D(g), p0[size_t(i)].y + D(g)} : Pt2{U(g), U(g)};
    Desc a{n0, 64, d0.data()}, b{n1, 64, d1.data()};
    std::vector<int> m0{-7}, m1{-7};  // the overload APPENDS (push_back), as the reference
    CHECK(sfm_compat::matchFeatures(p0, a, p1, b, m0, m1) == 0);
    CHECK(m0.size() == m1.size() && m0.size() > 100 && m0[0] == -7);
    std::printf("  matcher: %zu matches appended\n", m0.size() - 1);
    const int w = 320, h = 240;
    std::vector<uint8_t> img(size_t(w) * h), half(size_t(w / 2) * (h / 2));
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) img[size_t(y) * w + x] = uint8_t((x * 7 + y * 13 + ((x / 16 + y / 16) & 1) * 90) & 255);
    std::vector<float> eig(size_t(w) * h);
    oracle_min_eigen(img.data(), w, h, eig.data());
    oracle_pyr_down(img.data(), w, h, half.data());
    std::vector<int16_t> dxy(2 * size_t(w) * h);
    oracle_scharr(img.data(), w, h, dxy.data());
    std::printf("  gftt / pyramid / scharr ok\n");
  }
  std::printf("asan: all checks passed (%d checks)\n", g_checks);
  return 0;
}
