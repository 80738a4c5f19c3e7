// The culling members of sfm_compat::MapStore driven as CSfM::cullMapPoints /
// CSfM::cullKeyFrames drive CMap (CSfM.cpp:692-752): the pinned hand-checked
// case of tests/cull_cases.py, replayed through the C++ drop-in.  Every output
// is checked here against the same written-out expectations; the program
// prints "compat_cull_gpu ok" and returns 0 only when all of them hold.
// Usage: compat_cull_gpu [desc_bytes]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sfm_ctracker_compat.hpp"

namespace {

struct P3 {
  double val[3];
};
struct Desc {  // cv::Mat's members MapStore reads
  int rows, cols;
  const uint8_t* data;
};

int g_fail = 0;
using V = std::vector<int>;

void expect(bool ok, const char* what, int line) {
  if (!ok) {
    std::printf("FAILED line %d: %s (%s)\n", line, what, sfm_last_error());
    ++g_fail;
  }
}
#define EXPECT(c) expect((c), #c, __LINE__)

struct Driver {
  sfm_compat::MapStore m;
  int bytes;
  unsigned seed = 12345;
  explicit Driver(int b) : m(b), bytes(b) {}

  void rows(const V& pts) {
    std::vector<uint8_t> d(pts.size() * size_t(bytes));
    for (auto& x : d) {
      seed = seed * 1664525u + 1013904223u;
      x = uint8_t(seed >> 24);
    }
    Desc mat{int(pts.size()), bytes, d.data()};
    EXPECT(m.addDescriptors(pts, mat) == SFM_OK);
  }
  V newPoints(int n, const std::vector<V>& i2, const V& frames) {
    std::vector<P3> X(size_t(n), P3{{0.5, -1.0, 4.0}});
    V idx;
    EXPECT(m.addNewPoints(X, i2, frames, idx) == SFM_OK);
    return idx;
  }
  void matches(const V& pts, const V& i2, int f) {
    EXPECT(m.addPointMatches(pts, i2, f) == SFM_OK);
    rows(pts);
  }
  V state(const V& pts) {
    V s;
    EXPECT(m.pointState(pts, s) == SFM_OK);
    return s;
  }
  V cull(V* status) {
    V c;
    EXPECT(m.removePointsThreshold(c, *status) == SFM_OK);
    return c;
  }
  V cullKf(const V& fr, const std::vector<V>& lists, int nf, double rate) {
    V c;
    EXPECT(m.cullKeyFrames(fr, lists, nf, rate, c) == SFM_OK);
    return c;
  }
  void frame(int f, const V& want3, const V& want2) {
    V p3, p2;
    EXPECT(m.getPointsInFrame(p3, p2, f) == SFM_OK);
    EXPECT(p3 == want3);
    EXPECT(p2 == want2);
  }
};

V rep(const V& a, int k) {
  V out;
  for (int i = 0; i < k; ++i) out.insert(out.end(), a.begin(), a.end());
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  const int bytes = argc > 1 ? std::atoi(argv[1]) : 64;
  Driver d(bytes);
  if (d.m.status() != SFM_OK) {
    std::printf("sfm_map_create failed: %s\n", sfm_last_error());
    return 2;
  }
  V status;
  // 1. setup
  EXPECT(d.newPoints(6, {{10, 11, 12, 13, 14, 15}, {20, 21, 22, 23, 24, 25}}, {0, 5}) == (V{0, 1, 2, 3, 4, 5}));
  d.rows({0, 1, 2, 3, 4, 5});
  d.rows({0, 1, 2, 3, 4, 5});
  EXPECT(d.m.incrementMapAge(0, 2) == SFM_OK);
  V views = rep({0}, 10);
  for (const V& v : {V{2}, rep({3}, 2), rep({4}, 10), rep({5}, 10)}) views.insert(views.end(), v.begin(), v.end());
  EXPECT(d.m.updatePointViews(views) == SFM_OK);
  EXPECT(d.m.incrementMapAge(10, 0) == SFM_OK);
  d.matches({0, 2, 3, 4, 4, 5}, {30, 32, 33, 34, 35, 36}, 15);
  EXPECT(d.newPoints(2, {{16, 17}}, {0}) == (V{6, 7}));
  d.rows({6, 7});
  d.matches({6}, {26}, 5);
  d.matches({6, 7}, {37, 38}, 15);
  EXPECT(d.state({0, 1, 2, 3, 4, 5, 6, 7}) ==
         (V{10, 2, 13, 3, 1, 10, 2, 2, 2, 1, 10, 2, 4, 3, 1, 10, 2, 5, 3, 1, 10, 2, 14, 4, 1, 10, 2, 13, 3, 1,
            0, 0, 3, 3, 1, 0, 0, 2, 2, 1}));
  EXPECT(d.m.getNPoints() == 8 && d.m.getNSlots() == 8);
  // 2. first point cull
  EXPECT(d.cull(&status) == (V{1}));
  EXPECT(status == (V{0, -1, 0, 0, 0, 0, 0, 0}));
  EXPECT(d.m.getNPoints() == 7 && d.m.getNSlots() == 8);
  // 3. first keyframe cull
  EXPECT(d.cullKf({0, 5, 15}, {{0, 3, 4, 5, 6, 7}, {0, 3, 4, 5, 6}, {0, 3, 4, 4, 5, 6, 7}}, 3, 0.9) == (V{0, 0, 0}));
  EXPECT(d.m.incrementMapAge(0, 1) == SFM_OK);
  // 4. next keyframe
  EXPECT(d.m.incrementMapAge(10, 0) == SFM_OK);
  EXPECT(d.m.updatePointViews(rep({0, 3, 4, 5, 6}, 10)) == SFM_OK);
  d.matches({0, 3, 4, 5, 6}, {40, 43, 44, 45, 46}, 25);
  // 5. second point cull
  EXPECT(d.cull(&status) == (V{2, 7}));
  EXPECT(status == (V{0, 0, -1, 0, 0, 0, 0, -1}));
  // 6. second keyframe cull
  const V fr{0, 5, 15, 25};
  const std::vector<V> lists{{0, 3, 4, 5}, {0, 3, 4, 5, 6}, {0, 3, 4, 4, 5, 6}, {0, 3, 4, 5, 6}};
  bool seen = true;
  EXPECT(d.m.arePointsSeenByAtLeast(lists[0], 3, 0.9, seen) == SFM_OK && !seen);
  EXPECT(d.m.arePointsSeenByAtLeast(lists[0], 3, 0.5, seen) == SFM_OK && seen);
  EXPECT(d.cullKf(fr, lists, 3, 0.9) == (V{0, 0, 0, 0}));
  EXPECT(d.cullKf(fr, lists, 3, 0.5) == (V{1, 0, 0, 0}));
  EXPECT(d.state({0, 4, 6}) == (V{20, 3, 23, 3, 1, 20, 3, 24, 4, 1, 10, 1, 14, 4, 1}));
  d.frame(0, {}, {});
  V in0;
  EXPECT(d.m.getPointsInFrames(in0, {0}) == SFM_OK && in0.empty());
  d.frame(15, {0, 3, 4, 4, 5, 6}, {30, 33, 34, 35, 34, 35, 36, 37});
  d.frame(5, {0, 3, 4, 5, 6}, {20, 23, 24, 25, 26});
  d.frame(25, {0, 3, 4, 5, 6}, {40, 43, 44, 45, 46});
  // 7. third keyframe cull
  EXPECT(d.m.incrementMapAge(0, 1) == SFM_OK);
  EXPECT(d.cullKf({5, 15, 25}, {lists[1], lists[2], lists[3]}, 2, 0.0) == (V{1, 1, 0}));
  EXPECT(d.state({0, 3, 4, 5, 6}) ==
         (V{20, 4, 21, 1, 1, 20, 4, 13, 1, 1, 20, 4, 21, 1, 1, 20, 4, 21, 1, 1, 10, 2, 12, 2, 1}));
  d.frame(25, {0, 3, 4, 5, 6}, {40, 43, 44, 45, 46});
  d.frame(5, {}, {});
  d.frame(15, {}, {});
  // 8. third point cull
  EXPECT(d.cull(&status) == (V{0, 3, 4, 5, 6}));
  EXPECT(status == (V{-1, 0, 0, -1, -1, -1, -1, 0}));
  EXPECT(d.m.getNPoints() == 0 && d.m.getNSlots() == 8);
  d.frame(25, {}, {});
  int32_t np = 0;
  int64_t no = -1, nd = -1;
  EXPECT(sfm_map_size(d.m.handle(), &np, &no, &nd) == SFM_OK && np == 8 && no == 0 && nd == 0);
  // 9. error case: the point is gone, nothing changes
  EXPECT(d.m.removeFrame(15, {0}) == SFM_EINVAL);
  EXPECT(d.m.removePoints({0}, status) == SFM_EINVAL);
  EXPECT(d.m.getNPoints() == 0);
  if (g_fail) return 1;
  std::printf("compat_cull_gpu ok\n");
  return 0;
}
