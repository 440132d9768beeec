// Farthest-point sampling — utils/time_utils.py:461-482 of the reference, bit for bit: `nearest` starts at 1e10, the squared
// distance is fl(fl(dx dx + dy dy) + dz dz) (every product and sum rounded, no fused multiply-add: this unit is built with
// -ffp-contract=off), the update is `dist < nearest`, the next point is the maximum of `nearest` with the LOWEST index on ties
// (what torch.max returns on the CPU), and the output holds the start index first.
//
// One plain launch per picked point; no grid barrier, no cooperative launch, no workgroup waits on another.  Launch i:
//   1. every workgroup folds the (max, index) partials that launch i - 1 left — one per workgroup, in a fixed order, all
//      workgroups redundantly — into the current point (launch 0 reads the start index from a device word instead);
//      workgroup 0 writes it to out[i];
//   2. every workgroup updates `nearest` over its own contiguous slice of the points against the current point and writes the
//      slice's (max, lowest index) into the OTHER half of a double buffer of partials (the half launch i + 1 folds; the half
//      it reads is not written again before launch i + 2).
// Per launch: 12 B of position + 4 B of `nearest` read and up to 4 B written per point (6 MB at 300 k points, L2 / MALL
// resident from the second launch on), 8 B per workgroup of partials.  That is ~1-2 us of traffic: the sweep is bound by the
// launch boundary, not by bytes.
#include "common.h"

namespace riggs {

#define FPS_THREADS 256
#define FPS_MIN_SLICE 1024   // points per workgroup: N <= 1024 is one workgroup
#define FPS_MAX_BLOCKS 1024  // the fold reads one partial per workgroup: keep it a few loads per thread

struct FpsPartial { float v; int32_t i; };

static inline int fps_slice(int N) {
  long long per = ((long long)N + FPS_MAX_BLOCKS - 1) / FPS_MAX_BLOCKS;
  per = (per + FPS_THREADS - 1) / FPS_THREADS * FPS_THREADS;
  return (int)(per < FPS_MIN_SLICE ? FPS_MIN_SLICE : per);
}
static inline int fps_blocks(int N) { const int per = fps_slice(N); return N <= 0 ? 1 : (N + per - 1) / per; }

// the greater value wins; equal values: the lower index.  (an index < 0 is "nothing yet" and loses to everything)
__device__ __forceinline__ void fps_take(float& v, int& i, float ov, int oi) {
  if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
}

// (v, i) of the whole workgroup in every thread.  s: 2 x 4 words of LDS; two barriers.
__device__ __forceinline__ void fps_block_max(float& v, int& i, float* s_v, int* s_i) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    fps_take(v, i, ov, oi);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_v[wave] = v; s_i[wave] = i; }
  __syncthreads();
  v = s_v[0]; i = s_i[0];
#pragma unroll
  for (int w = 1; w < FPS_THREADS / 64; w++) fps_take(v, i, s_v[w], s_i[w]);
  __syncthreads();
}

__global__ __launch_bounds__(FPS_THREADS) void fps_step_kernel(int N, int step, int last, int slice, int n_blocks,
                                                               const float* __restrict__ xyz, long long row_stride,
                                                               const long long* __restrict__ start, float* __restrict__ nearest,
                                                               FpsPartial* __restrict__ partials /* (2, n_blocks) */,
                                                               long long* __restrict__ out) {
  __shared__ float s_v[FPS_THREADS / 64];
  __shared__ int s_i[FPS_THREADS / 64];
  const int tid = threadIdx.x;
  int cur;
  if (step == 0) {
    const long long s = start[0];
    cur = (int)(s < 0 ? 0 : (s >= N ? N - 1 : s));   // (an index outside the cloud is clamped: nothing is read past it)
  } else {
    const FpsPartial* __restrict__ prev = partials + (size_t)((step - 1) & 1) * n_blocks;
    float v = 0.0f;
    int i = -1;
    for (int b = tid; b < n_blocks; b += FPS_THREADS) {   // ascending blocks = ascending indices: ties keep the lower
      const FpsPartial p = prev[b];
      fps_take(v, i, p.v, p.i);
    }
    fps_block_max(v, i, s_v, s_i);
    cur = i < 0 ? 0 : (i >= N ? N - 1 : i);
  }
  if (blockIdx.x == 0 && tid == 0) out[step] = cur;
  if (last) return;   // the last pick needs no further sweep

  const float cx = xyz[(size_t)cur * row_stride], cy = xyz[(size_t)cur * row_stride + 1], cz = xyz[(size_t)cur * row_stride + 2];
  const int lo = blockIdx.x * slice;
  const int hi = lo + slice < N ? lo + slice : N;
  float best = 0.0f;
  int best_i = -1;
  for (int n = lo + tid; n < hi; n += FPS_THREADS) {
    const float* __restrict__ p = xyz + (size_t)n * row_stride;
    const float dx = p[0] - cx, dy = p[1] - cy, dz = p[2] - cz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    float m = step == 0 ? 1e10f : nearest[n];
    if (d < m) m = d;
    nearest[n] = m;
    if (best_i < 0 || m > best) { best = m; best_i = n; }   // n ascends: strict > keeps the lower index
  }
  fps_block_max(best, best_i, s_v, s_i);
  if (tid == 0) {
    FpsPartial p;
    p.v = best; p.i = best_i;
    partials[(size_t)(step & 1) * n_blocks + blockIdx.x] = p;
  }
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int32_t riggs_fps_blocks(int32_t N) { return fps_blocks(N); }

size_t riggs_fps_workspace_bytes(int32_t N) {
  const size_t n = N > 0 ? (size_t)N : 1;
  return align_up(n * sizeof(float)) + align_up(2 * (size_t)fps_blocks(N) * sizeof(FpsPartial));
}

int riggs_fps_sample(int32_t N, int32_t npoint, const float* xyz, int64_t row_stride, const int64_t* start, void* workspace,
                     int64_t* out_indices, riggs_stream stream) {
  RIGGS_REQUIRE(N >= 1 && npoint >= 0 && row_stride >= 3, "riggs_fps_sample: needs N >= 1, npoint >= 0 and a row stride of at least 3 floats");
  if (npoint == 0) return 0;
  RIGGS_REQUIRE(xyz && start && workspace && out_indices, "riggs_fps_sample: NULL argument");
  const int slice = fps_slice(N), nb = fps_blocks(N);
  float* nearest = (float*)workspace;
  FpsPartial* partials = (FpsPartial*)((char*)workspace + align_up((size_t)N * sizeof(float)));
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < npoint; i++) {
    const int last = i == npoint - 1;
    hipLaunchKernelGGL(fps_step_kernel, dim3(last ? 1 : nb), dim3(FPS_THREADS), 0, s, (int)N, i, last, slice, nb, xyz,
                       (long long)row_stride, (const long long*)start, nearest, partials, (long long*)out_indices);
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
