// Read-only view of the device map store (map_store.hip) for the stages that
// read the map's points where they live.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/sfm_amd.h"

namespace sfm {
struct MapPointsView {
  const double* X;      // [n_slots][3]; a removed point keeps its slot
  const uint8_t* live;  // [n_slots]; 1: the point is in _pts3DIdx
  int32_t n_slots;      // ascending slot = _pts3DIdx order
  int32_t n_live;
  int device;
  hipStream_t stream;   // the map's pending work, if any, sits here
};
MapPointsView map_points_view(sfm_map* h);
}  // namespace sfm
