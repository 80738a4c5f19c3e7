// The camera templates of include/sfm_ctracker_compat.hpp against stub types
// (no OpenCV, no GPU): prints Kopt of the lens given on the command line as
// hex floats for tests/test_compat_camera.py to compare with the restatement.
//   compat_camera_check W H fx fy cx cy [d...]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sfm_ctracker_compat.hpp"

struct Matx33d { double val[9]; };
struct Size { int width, height; };
struct Point2d { double x, y; };

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const Size sz{std::atoi(argv[1]), std::atoi(argv[2])};
  const Matx33d K{{std::strtod(argv[3], nullptr), 0, std::strtod(argv[5], nullptr), 0, std::strtod(argv[4], nullptr),
                   std::strtod(argv[6], nullptr), 0, 0, 1}};
  std::vector<double> d;
  for (int i = 7; i < argc; ++i) d.push_back(std::strtod(argv[i], nullptr));
  Matx33d Kopt{{-1, -1, -1, -1, -1, -1, -1, -1, -1}};
  const int rc = sfm_compat::getOptimalNewCameraMatrix(K, d, sz, Kopt);
  std::printf("rc %d\n", rc);
  for (int m = 0; m < 9; ++m) std::printf("%a ", Kopt.val[m]);
  std::printf("\n");
  // no points: succeeds without a device; a bad coefficient count does not
  std::vector<Point2d> none, out(3);
  const int rc0 = sfm_compat::undistortPoints(none, out, K, d, Kopt);
  std::vector<Point2d> one(1, Point2d{10.0, 20.0});
  const int rc1 = sfm_compat::undistortPoints(one, out, K, std::vector<double>(3, 0.0), Kopt);
  std::printf("empty %d size %zu bad %d\n", rc0, out.size(), rc1);
  return 0;
}
