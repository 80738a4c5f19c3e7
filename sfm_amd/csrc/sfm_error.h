// The calling thread's last error, as every translation unit reports it.
// No HIP includes: the host-only files (camera.cpp, scene.cpp,
// guidance_host.cpp) use this too.
#pragma once
#include <string>

void sfm_internal_set_error(const std::string& msg);  // ba_solver.hip holds the message

inline int fail(int code, const std::string& msg) {
  sfm_internal_set_error(msg);
  return code;
}
