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
//
// The same step (fps_step) runs over rows of up to 64 floats — riggs_fps_sample_rows, the sampling of stage-1 control nodes by
// their trajectories — with another way of reading a point: see FpsColumns below.
#include "common.h"

namespace riggs {

#define FPS_THREADS 256
#define FPS_MIN_SLICE 1024   // points per workgroup (3-column clouds): N <= 1024 is one workgroup
#define FPS_MAX_BLOCKS 1024  // the fold reads one partial per workgroup: keep it a few loads per thread

struct FpsPartial { float v; int32_t i; };

static inline int fps_slice(int N, int min_slice = FPS_MIN_SLICE) {
  long long per = ((long long)N + FPS_MAX_BLOCKS - 1) / FPS_MAX_BLOCKS;
  per = (per + FPS_THREADS - 1) / FPS_THREADS * FPS_THREADS;
  return (int)(per < min_slice ? min_slice : per);
}
static inline int fps_blocks(int N, int min_slice = FPS_MIN_SLICE) {
  const int per = fps_slice(N, min_slice);
  return N <= 0 ? 1 : (N + per - 1) / per;
}

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

// One step of the sweep over a cloud of any layout.  Cloud: set_current(cur) makes point `cur` the current one (every thread of the
// workgroup calls it), dist(n) is the squared distance of point n to it.
template <class Cloud>
__device__ __forceinline__ void fps_step(int N, int step, int last, int slice, int n_blocks, Cloud& cloud,
                                         const long long* __restrict__ start, float* __restrict__ nearest,
                                         FpsPartial* __restrict__ partials /* (2, n_blocks) */, long long* __restrict__ out) {
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

  cloud.set_current(cur);
  const int lo = blockIdx.x * slice;
  const int hi = lo + slice < N ? lo + slice : N;
  float best = 0.0f;
  int best_i = -1;
  for (int n = lo + tid; n < hi; n += FPS_THREADS) {
    const float d = cloud.dist(n);
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

// rows of 3 floats read in place: 12 B per point, the current point in three registers
struct FpsXyz {
  const float* __restrict__ xyz;
  long long row_stride;
  float cx, cy, cz;
  __device__ __forceinline__ void set_current(int cur) {
    cx = xyz[(size_t)cur * row_stride]; cy = xyz[(size_t)cur * row_stride + 1]; cz = xyz[(size_t)cur * row_stride + 2];
  }
  __device__ __forceinline__ float dist(int n) const {
    const float* __restrict__ p = xyz + (size_t)n * row_stride;
    const float dx = p[0] - cx, dy = p[1] - cy, dz = p[2] - cz;
    return (dx * dx + dy * dy) + dz * dz;
  }
};

__global__ __launch_bounds__(FPS_THREADS) void fps_step_kernel(int N, int step, int last, int slice, int n_blocks,
                                                               const float* __restrict__ xyz, long long row_stride,
                                                               const long long* __restrict__ start, float* __restrict__ nearest,
                                                               FpsPartial* __restrict__ partials, long long* __restrict__ out) {
  FpsXyz cloud = {xyz, row_stride, 0.0f, 0.0f, 0.0f};
  fps_step(N, step, last, slice, n_blocks, cloud, start, nearest, partials, out);
}

// ---- rows of D floats, 1 <= D <= FPS_MAX_WIDTH (the stage-1 node sampling: 16 time samples of a trajectory, D = 48) ------------
// Squared distance: the sequential fp32 sum ((t_0^2 + t_1^2) + t_2^2) + ... over ascending columns, t_k = fl(p_k - c_k), every
// product and sum rounded — at D = 3 what FpsXyz computes.
// Layout: the rows are transposed ONCE per call into a (D, N) image in the workspace (fps_transpose_kernel), and one thread then
// walks one point down the D columns: every wave load is 64 consecutive floats of one column, so each 128-B line that is fetched
// is used whole.  Two layouts were built and timed on one MI355X (profiles/fps_rows_layouts.json); the other one
// read the (N, D) rows in place, a tile of 256 whole rows staged through LDS with consecutive lanes on consecutive floats and
// then one thread per row out of LDS at an odd pitch.  This one won at both sizes: 13.3 against 17.5 us per pick at
// 300 000 x 48 and 5.2 against 7.6 us at 20 000 x 48, and needs no LDS tile; it costs 4 N D bytes of workspace.
// Per launch: 4 D + 4 B read and up to 4 B written per point (57.6 MB + 1.2 MB at 300 000 x 48: Infinity Cache resident); the
// transposition reads and writes the cloud once more, per call.  The current point's row (uniform across the grid) is copied from
// the caller's rows (D consecutive floats) into LDS once per workgroup and read back as 16-byte broadcasts.
// Slices: 256 points per workgroup at least (one per thread) — at 1 024, the 3-column kernel's, 20 000 x 48 took 7.7 us per pick.
#define FPS_MAX_WIDTH 64
#define FPS_ROWS_MIN_SLICE 256   // points per workgroup at least
#define FPS_TR_ROWS 64           // rows per workgroup of the transposition

__global__ __launch_bounds__(FPS_THREADS) void fps_transpose_kernel(int N, int D, const float* __restrict__ rows, long long row_stride,
                                                                    float* __restrict__ image /* (D, N) */) {
  __shared__ float s[FPS_MAX_WIDTH][FPS_TR_ROWS + 1];
  const long long n0 = (long long)blockIdx.x * FPS_TR_ROWS;
  const int cnt = N - n0 < FPS_TR_ROWS ? (int)(N - n0) : FPS_TR_ROWS;
  for (int e = threadIdx.x; e < cnt * D; e += FPS_THREADS) {   // consecutive threads: consecutive floats of a row
    const int r = e / D, k = e - r * D;
    s[k][r] = rows[(size_t)(n0 + r) * row_stride + k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < D * FPS_TR_ROWS; e += FPS_THREADS) {   // consecutive threads: consecutive points of a column
    const int k = e / FPS_TR_ROWS, r = e - k * FPS_TR_ROWS;
    if (r < cnt) image[(size_t)k * N + n0 + r] = s[k][r];
  }
}

struct FpsColumns {
  const float* __restrict__ rows;    // (N, D), row_stride floats apart: the current point is read from here
  long long row_stride;
  const float* __restrict__ image;   // (D, N)
  int N, D;
  float* s_c;                        // FPS_MAX_WIDTH floats of LDS, 16-byte aligned
  __device__ __forceinline__ void set_current(int cur) {
    if ((int)threadIdx.x < D) s_c[threadIdx.x] = rows[(size_t)cur * row_stride + threadIdx.x];
    __syncthreads();
  }
  __device__ __forceinline__ float dist(int n) const {
    const float* __restrict__ p = image + n;
    float acc = 0.0f;   // (0 + t_0^2 is t_0^2)
    int k = 0;
#pragma unroll 4
    for (; k + 4 <= D; k += 4) {
      const float4 c = *(const float4*)(s_c + k);
      const float p0 = p[(size_t)k * N], p1 = p[(size_t)(k + 1) * N], p2 = p[(size_t)(k + 2) * N], p3 = p[(size_t)(k + 3) * N];
      const float t0 = p0 - c.x, t1 = p1 - c.y, t2 = p2 - c.z, t3 = p3 - c.w;
      acc += t0 * t0; acc += t1 * t1; acc += t2 * t2; acc += t3 * t3;
    }
    for (; k < D; k++) {
      const float t = p[(size_t)k * N] - s_c[k];
      acc += t * t;
    }
    return acc;
  }
};

__global__ __launch_bounds__(FPS_THREADS) void fps_rows_step_kernel(int N, int D, int step, int last, int slice, int n_blocks,
                                                                    const float* __restrict__ rows, long long row_stride,
                                                                    const float* __restrict__ image,
                                                                    const long long* __restrict__ start, float* __restrict__ nearest,
                                                                    FpsPartial* __restrict__ partials, long long* __restrict__ out) {
  __shared__ __align__(16) float s_c[FPS_MAX_WIDTH];
  FpsColumns cloud = {rows, row_stride, image, N, D, s_c};
  fps_step(N, step, last, slice, n_blocks, cloud, start, nearest, partials, out);
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

size_t riggs_fps_rows_workspace_bytes(int32_t N, int32_t D) {
  const size_t n = N > 0 ? (size_t)N : 1, d = D > 0 ? (size_t)D : 1;
  return align_up(n * sizeof(float)) + align_up(2 * (size_t)fps_blocks(N, FPS_ROWS_MIN_SLICE) * sizeof(FpsPartial)) +
         align_up(n * d * sizeof(float));
}

int riggs_fps_sample_rows(int32_t N, int32_t D, int32_t npoint, const float* rows, int64_t row_stride, const int64_t* start,
                          void* workspace, int64_t* out_indices, riggs_stream stream) {
  RIGGS_REQUIRE(D >= 1 && D <= FPS_MAX_WIDTH, "riggs_fps_sample_rows: rows of 1 to 64 floats");
  RIGGS_REQUIRE(N >= 1 && npoint >= 0 && row_stride >= D, "riggs_fps_sample_rows: needs N >= 1, npoint >= 0 and a row stride of at least D floats");
  if (npoint == 0) return 0;
  RIGGS_REQUIRE(rows && start && workspace && out_indices, "riggs_fps_sample_rows: NULL argument");
  const int slice = fps_slice(N, FPS_ROWS_MIN_SLICE), nb = fps_blocks(N, FPS_ROWS_MIN_SLICE);
  float* nearest = (float*)workspace;
  FpsPartial* partials = (FpsPartial*)((char*)nearest + align_up((size_t)N * sizeof(float)));
  float* image = (float*)((char*)partials + align_up(2 * (size_t)nb * sizeof(FpsPartial)));
  hipStream_t s = (hipStream_t)stream;
  if (npoint > 1)   // (a single pick is the start index: no sweep reads the image)
    hipLaunchKernelGGL(fps_transpose_kernel, dim3((unsigned)(((long long)N + FPS_TR_ROWS - 1) / FPS_TR_ROWS)), dim3(FPS_THREADS), 0, s,
                       (int)N, (int)D, rows, (long long)row_stride, image);
  for (int i = 0; i < npoint; i++) {
    const int last = i == npoint - 1;
    hipLaunchKernelGGL(fps_rows_step_kernel, dim3(last ? 1 : nb), dim3(FPS_THREADS), 0, s, (int)N, (int)D, i, last, slice, nb, rows,
                       (long long)row_stride, (const float*)image, (const long long*)start, nearest, partials, (long long*)out_indices);
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
