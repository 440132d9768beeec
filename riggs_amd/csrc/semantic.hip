// A semantic label per control node, for the symmetry pass of the skeleton extraction (riggs_amd/skeleton_init.py): what the
// reference's trainer collects camera by camera while it evaluates the trained stage 1 at every training frame
//   TrainRig.init_skeleton_info      train_rig.py:129-131   nodes_semantic_label = zeros(F, node_num)
//   project_nodes_to_2d_elements     utils/other_utils.py:101-127 (pinhole.h: the projection of skel_loss.hip)
//   TrainRig.set_semantic_label      train_rig.py:177-190   .long(), the three clamps, the gather; cameras without a map keep 0
//   torch.median(dim=0).values.int() train_rig.py:227       the LOWER median over the frames
// for all F frames in one launch.  Runs once per training run, F M ~ 10^5: sized for latency, not for throughput.
//
// A workgroup of 256 threads takes a tile of T nodes, T = the largest power of two <= 256 with F T words <= 64 KiB of LDS
// (F <= 64: 256, <= 128: 128, <= 256: 64, <= 512: 32, <= 1024: 16; 64 KiB of the CU's 160 so that two workgroups fit a CU).
//   1. the F T (frame, node) pairs of the tile, strided over the threads, consecutive threads on consecutive nodes: project,
//      truncate, clamp, gather; the label goes to labels[f][m] and, as the float the reference stores, to LDS at f T + t (F-major).
//   2. thread (g, t), g < 256 / T, takes node t and the candidate frames f = g, g + 256 / T, ...: the rank of candidate f is the
//      number of frames with a smaller label plus the number with an equal label and a smaller f — the ranks of a node are a
//      permutation of 0 .. F - 1, so exactly one candidate has rank (F - 1) / 2 and its thread writes the median.  The F-loop
//      reads LDS at k T + t: consecutive lanes read consecutive words, lanes that share t (T < 64) the same word — no bank
//      conflicts.  Exact and deterministic: no sort network, no atomics.
#include "common.h"
#include "pinhole.h"

#include <stddef.h>

namespace riggs {

#define SEM_THREADS 256
#define SEM_LDS_WORDS (64 * 1024 / 4)

// a camera record as the header lays it out in words
struct SemCamera {
  float view[16];
  float fx, fy, cx, cy;
  int32_t H, W;
  const int32_t* map;
};
static_assert(sizeof(SemCamera) == RIGGS_SEMANTIC_CAMERA_WORDS * 4 && offsetof(SemCamera, H) == 80 && offsetof(SemCamera, map) == 88,
              "SemCamera is the record of include/riggs_hip.h");

static inline int sem_tile(int F) {
  int T = SEM_THREADS;
  while (T * F > SEM_LDS_WORDS) T >>= 1;  // F <= 1024: T >= 16
  return T;
}

// trunc(x) clamped as the reference clamps it (>= n -> n - 1 first, then < 0 -> 0), without forming an integer that may not
// fit: trunc(x) >= n iff x >= n, trunc(x) < 0 iff x <= -1.  x is finite.
__device__ __forceinline__ int sem_pixel(float x, int n) { return x >= (float)n ? n - 1 : (x <= -1.0f ? 0 : (int)x); }

__global__ __launch_bounds__(SEM_THREADS) void semantic_labels_kernel(int F, int M, int T, int logT, const float* __restrict__ d_nodes,
                                                                      const SemCamera* __restrict__ cams,
                                                                      float* __restrict__ labels, int32_t* __restrict__ median) {
  extern __shared__ float sem_lds[];  // (F, T)
  const int tid = threadIdx.x, m0 = blockIdx.x * T;
  for (int i = tid; i < F * T; i += SEM_THREADS) {
    const int f = i >> logT, m = m0 + (i & (T - 1));
    int32_t v = 0;
    if (m < M) {
      const SemCamera& c = cams[f];
      if (c.map && c.H >= 1 && c.W >= 1) {
        const float* p = d_nodes + ((size_t)f * M + m) * 3;
        float tx, ty, tz;
        pinhole_view(c.view, p[0], p[1], p[2], tx, ty, tz);
        const float2 rc = pinhole_row_col(c.fx, c.fy, c.cx, c.cy, tx, ty, tz);
        int row = 0, col = 0;
        if (isfinite(rc.x) && isfinite(rc.y)) { row = sem_pixel(rc.x, c.H); col = sem_pixel(rc.y, c.W); }
        v = c.map[(size_t)row * c.W + col];
      }
      labels[(size_t)f * M + m] = (float)v;
    }
    sem_lds[i] = (float)v;
  }
  __syncthreads();
  const int t = tid & (T - 1), g = tid >> logT, G = SEM_THREADS >> logT, m = m0 + t, want = (F - 1) / 2;
  if (m >= M) return;
  for (int f = g; f < F; f += G) {
    const float v = sem_lds[f * T + t];
    int rank = 0;
    for (int k = 0; k < F; k++) {
      const float u = sem_lds[k * T + t];
      rank += (int)((u < v) | ((u == v) & (k < f)));
    }
    if (rank == want) median[m] = (int32_t)v;
  }
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int32_t riggs_node_semantic_tile(int32_t F) { return F >= 1 && F <= RIGGS_SEMANTIC_MAX_FRAMES ? sem_tile(F) : 0; }

int riggs_node_semantic_labels(int32_t F, int32_t M, const float* d_nodes, const void* cameras, float* labels, int32_t* median,
                               riggs_stream stream) {
  RIGGS_REQUIRE(F >= 1 && F <= RIGGS_SEMANTIC_MAX_FRAMES && M >= 1 && M <= RIGGS_SEMANTIC_MAX_NODES,
                "riggs_node_semantic_labels: needs 1 <= F <= 1024 frames and 1 <= M <= 65536 nodes");
  RIGGS_REQUIRE(d_nodes && cameras && labels && median, "riggs_node_semantic_labels: NULL argument");
  RIGGS_REQUIRE(((uintptr_t)cameras & 7u) == 0, "riggs_node_semantic_labels: the camera table must be 8-byte aligned");
  const int T = sem_tile(F);
  int logT = 0;
  while ((1 << logT) < T) logT++;
  hipLaunchKernelGGL(semantic_labels_kernel, dim3((M + T - 1) / T), dim3(SEM_THREADS), (size_t)F * T * sizeof(float),
                     (hipStream_t)stream, (int)F, (int)M, T, logT, d_nodes, (const SemCamera*)cameras, labels, median);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
