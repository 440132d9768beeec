// The pinhole of project_nodes_to_2d_elements (utils/other_utils.py:101-127), shared by the projection losses (skel_loss.hip) and
// the nodes' semantic labels (semantic.hip) so that both see the same pixel for the same point: one fp32 operation order, and
// both translation units are built without FP contraction.
#pragma once
#include "common.h"

namespace riggs {

// World point -> camera space; V: (4, 4) world_view_transform as the reference stores it (row-vector convention).
__device__ __forceinline__ void pinhole_view(const float* V,float px, float py, float pz, float& tx, float& ty, float& tz) {
  tx = px * V[0] + py * V[4] + pz * V[8] + V[12];
  ty = px * V[1] + py * V[5] + pz * V[9] + V[13];
  tz = px * V[2] + py * V[6] + pz * V[10] + V[14];
}

// (row, col) of a camera-space point
__device__ __forceinline__ float2 pinhole_row_col(float fx, float fy, float cx, float cy, float tx, float ty, float tz) {
  return make_float2(fy * ty / tz + cy, fx * tx / tz + cx);
}

}  // namespace riggs
