// Multiresolution hash-grid encoding (Mueller et al., Instant Neural Graphics Primitives, 2022): the input encoding of the
// reference's HashDeformNetwork, which takes it from tinycudann.Encoding.  Restated from the published algorithm (the arithmetic is
// spelled out in include/riggs_hip.h and restated in NumPy in tests/hashgrid_ref.py); agreement with tinycudann's binary is NOT
// verified — it does not build for this platform.
//
// WORKGROUP = 64 rows x L levels: wave w serves level w, lane k row r0 + k.  The lanes of a wave share a level, so they share its
// scale, resolution and table window (a coarse level's window is a few KiB: L2-resident), and an entry's two features are one
// 8-byte access.  A row's L F outputs come from L different waves; they meet in an LDS tile (64 x L F floats, 8 KiB at most) that
// the whole workgroup then copies out as one contiguous run of full rows — and, in the backward, copies in the same way.
//
// BACKWARD: the only gradient is the table's.  Each (row, level, corner, feature) is one float atomic add (a single
// global_atomic_add_f32, no compare-and-swap loop); a node query adds 512 x 12 x 8 x 2 floats, the node-Gaussian stage 65 536 rows
// of the same: far below the chip-wide atomic rate, so nothing is pre-summed.  The sum's order is the arrival order: the gradient
// can differ in its last bits from run to run.  The coordinates are not differentiated.
//
// Every table index is taken modulo the level's size, so no coordinate — outside [0, 1], infinite or NaN — can address outside
// the level's window.  (A hashed level's size is 2^log2_hashmap_size: the modulo is a mask.  A dense level's index is below its
// size for every in-range cell: the division runs only for coordinates outside the grid.)
#include "common.h"

#include <math.h>

namespace riggs {

#define HG_ROWS 64
#define HG_MAX_L RIGGS_HASHGRID_MAX_LEVELS

struct HgLevels {
  float scale[HG_MAX_L];
  uint32_t res[HG_MAX_L], size[HG_MAX_L], offset[HG_MAX_L];
  uint32_t hashed;   // bit l: level l is hashed
};

template <int D>
struct HgCell {
  uint32_t cell[D];
  float frac[D];
};

template <int D>
__device__ __forceinline__ HgCell<D> hg_cell(const float* __restrict__ x, float scale) {
  HgCell<D> c;
#pragma unroll
  for (int d = 0; d < D; d++) {
    const float pos = __builtin_fmaf(scale, x[d], 0.5f), fl = floorf(pos);
    c.cell[d] = (uint32_t)(int32_t)fl;
    c.frac[d] = pos - fl;
  }
  return c;
}

// the weight and the table entry of corner `corner` (bit d: +1 along d)
template <int D>
__device__ __forceinline__ uint32_t hg_corner(const HgCell<D>& c, int corner, uint32_t res, uint32_t size, bool hashed, float& w) {
  const uint32_t primes[4] = {1u, 2654435761u, 805459861u, 3674653429u};
  uint32_t idx = 0u, stride = 1u;
  w = 1.0f;
#pragma unroll
  for (int d = 0; d < D; d++) {
    const uint32_t bit = (uint32_t)(corner >> d) & 1u, cd = c.cell[d] + bit;
    w *= bit ? c.frac[d] : 1.0f - c.frac[d];
    if (hashed) {
      idx ^= cd * primes[d];
    } else {
      idx += cd * stride;
      stride *= res;
    }
  }
  if (hashed) return idx & (size - 1u);   // (size = 2^log2_hashmap_size on every hashed level)
  return idx < size ? idx : idx % size;
}

template <int D>
__global__ void __launch_bounds__(HG_ROWS* HG_MAX_L)
hashgrid_forward_kernel(HgLevels lv, int L, int R, const float* __restrict__ x, const float2* __restrict__ table,
                        const float* __restrict__ mask, float2* __restrict__ out) {
  __shared__ float2 tile[HG_ROWS * HG_MAX_L];
  const int level = threadIdx.x / RIGGS_WAVE, lane = threadIdx.x % RIGGS_WAVE;
  const int r0 = blockIdx.x * HG_ROWS, row = r0 + lane;
  if (row < R) {
    const float m0 = mask ? mask[2 * level] : 1.0f, m1 = mask ? mask[2 * level + 1] : 1.0f;
    float2 acc = make_float2(0.0f, 0.0f);
    if (m0 != 0.0f || m1 != 0.0f) {
      const HgCell<D> c = hg_cell<D>(x + (size_t)row * D, lv.scale[level]);
      const uint32_t res = lv.res[level], size = lv.size[level];
      const bool hashed = (lv.hashed >> level) & 1u;
      const float2* __restrict__ tl = table + lv.offset[level];
#pragma unroll
      for (int k = 0; k < (1 << D); k++) {
        float w;
        const float2 v = tl[hg_corner<D>(c, k, res, size, hashed, w)];
        acc.x += w * v.x;
        acc.y += w * v.y;
      }
      acc.x *= m0;
      acc.y *= m1;
    }
    tile[lane * L + level] = acc;
  }
  __syncthreads();
  const int n = min(HG_ROWS, R - r0) * L;   // float2 elements of this workgroup's rows: one contiguous run
  float2* __restrict__ dst = out + (size_t)r0 * L;
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = tile[i];
}

template <int D>
__global__ void __launch_bounds__(HG_ROWS* HG_MAX_L)
hashgrid_backward_kernel(HgLevels lv, int L, int R, const float* __restrict__ x, const float* __restrict__ mask,
                         const float2* __restrict__ g_out, float2* __restrict__ g_table) {
  __shared__ float2 tile[HG_ROWS * HG_MAX_L];
  const int level = threadIdx.x / RIGGS_WAVE, lane = threadIdx.x % RIGGS_WAVE;
  const int r0 = blockIdx.x * HG_ROWS, row = r0 + lane;
  const int n = min(HG_ROWS, R - r0) * L;
  const float2* __restrict__ src = g_out + (size_t)r0 * L;
  for (int i = threadIdx.x; i < n; i += blockDim.x) tile[i] = src[i];
  __syncthreads();
  if (row >= R) return;
  const float m0 = mask ? mask[2 * level] : 1.0f, m1 = mask ? mask[2 * level + 1] : 1.0f;
  if (m0 == 0.0f && m1 == 0.0f) return;
  float2 g = tile[lane * L + level];
  g.x *= m0;
  g.y *= m1;
  const HgCell<D> c = hg_cell<D>(x + (size_t)row * D, lv.scale[level]);
  const uint32_t res = lv.res[level], size = lv.size[level];
  const bool hashed = (lv.hashed >> level) & 1u;
  float2* __restrict__ tl = g_table + lv.offset[level];
#pragma unroll
  for (int k = 0; k < (1 << D); k++) {
    float w;
    float* p = (float*)(tl + hg_corner<D>(c, k, res, size, hashed, w));
    atomicAdd(p, w * g.x);
    atomicAdd(p + 1, w * g.y);
  }
}

#define HG_HEAD RIGGS_HASHGRID_HEADER_WORDS
#define HG_LW RIGGS_HASHGRID_LEVEL_WORDS

// The host table (include/riggs_hip.h) into the kernels' argument; everything the kernels' bounds rest on is checked here.
static int hg_check(const uint32_t* lv, HgLevels& k, int& D, int& L, const char*& why) {
  why = "riggs_hashgrid: NULL levels";
  if (!lv) return 1;
  why = "riggs_hashgrid: levels were not filled by riggs_hashgrid_levels_fill (D in {3, 4}, 1 <= L <= 16, F = 2, log2_hashmap_size in 3 .. 24)";
  if ((lv[0] != 3u && lv[0] != 4u) || lv[1] < 1u || lv[1] > (uint32_t)HG_MAX_L || lv[2] != 2u || lv[3] < 3u || lv[3] > 24u) return 1;
  D = (int)lv[0]; L = (int)lv[1];
  const uint32_t cap = 1u << lv[3];
  // every level's window lies inside the table (the offsets are the running sum), a hashed size is the power of two
  uint32_t at = 0u;
  k.hashed = 0u;
  for (int l = 0; l < L; l++) {
    const uint32_t* w = lv + HG_HEAD + HG_LW * l;
    const uint32_t res = w[1], size = w[2], off = w[3], hashed = w[4];
    if (off != at || size < 8u || size > cap || res < 1u || hashed > 1u) return 1;
    if (hashed && size != cap) return 1;
    memcpy(&k.scale[l], &w[0], sizeof(float));
    k.res[l] = res; k.size[l] = size; k.offset[l] = at;
    k.hashed |= hashed << l;
    at += size;
  }
  if (lv[4] != at) return 1;
  for (int l = L; l < HG_MAX_L; l++) { k.scale[l] = 0.0f; k.res[l] = 1u; k.size[l] = 8u; k.offset[l] = 0u; }
  return 0;
}

static bool hg_aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_hashgrid_levels_fill(int32_t n_input_dims, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size,
                               double base_resolution, double per_level_scale, uint32_t* levels) {
  RIGGS_REQUIRE(levels, "riggs_hashgrid_levels_fill: NULL levels");
  RIGGS_REQUIRE(n_input_dims == 3 || n_input_dims == 4, "riggs_hashgrid_levels_fill: n_input_dims must be 3 or 4");
  RIGGS_REQUIRE(n_levels >= 1 && n_levels <= HG_MAX_L, "riggs_hashgrid_levels_fill: n_levels must be in 1 .. 16");
  RIGGS_REQUIRE(n_features_per_level == 2, "riggs_hashgrid_levels_fill: n_features_per_level must be 2");
  RIGGS_REQUIRE(log2_hashmap_size >= 3 && log2_hashmap_size <= 24, "riggs_hashgrid_levels_fill: log2_hashmap_size must be in 3 .. 24");
  RIGGS_REQUIRE(base_resolution >= 1.0 && per_level_scale >= 1.0, "riggs_hashgrid_levels_fill: base_resolution and per_level_scale must be >= 1");
  memset(levels, 0, RIGGS_HASHGRID_TABLE_WORDS * sizeof(uint32_t));
  levels[0] = (uint32_t)n_input_dims; levels[1] = (uint32_t)n_levels;
  levels[2] = (uint32_t)n_features_per_level; levels[3] = (uint32_t)log2_hashmap_size;
  const uint64_t cap = 1ull << log2_hashmap_size;
  uint32_t at = 0u;
  for (int l = 0; l < n_levels; l++) {
    const float scale = (float)(base_resolution * pow(per_level_scale, (double)l) - 1.0);
    RIGGS_REQUIRE(scale >= 0.0f && scale < 1073741824.0f, "riggs_hashgrid_levels_fill: a level's resolution must stay below 2^30");
    const uint32_t res = (uint32_t)ceilf(scale) + 1u;
    uint64_t cells = 1ull;   // res^D, exact while it matters: saturated far above any table size
    for (int d = 0; d < n_input_dims; d++) { cells *= res; if (cells > (1ull << 32)) cells = 1ull << 32; }
    uint64_t size = (cells + 7ull) / 8ull * 8ull;
    if (size > cap) size = cap;
    uint32_t* w = levels + HG_HEAD + HG_LW * l;
    memcpy(&w[0], &scale, sizeof(float));
    w[1] = res; w[2] = (uint32_t)size; w[3] = at; w[4] = cells > size ? 1u : 0u;
    at += (uint32_t)size;
  }
  levels[4] = at;
  return 0;
}

int riggs_hashgrid_forward(const uint32_t* levels, int32_t R, const float* x, const float* table, const float* mask,
                           float* out, riggs_stream stream) {
  HgLevels k; const char* why; int D = 0, L = 0;
  RIGGS_REQUIRE(hg_check(levels, k, D, L, why) == 0, why);
  RIGGS_REQUIRE(R >= 0 && (int64_t)R * 2 * L < (1ll << 31), "riggs_hashgrid_forward: needs 0 <= R < 2^31 / (L F)");
  if (R == 0) return 0;
  RIGGS_REQUIRE(x && table && out, "riggs_hashgrid_forward: NULL argument");
  RIGGS_REQUIRE(hg_aligned8(table) && hg_aligned8(out), "riggs_hashgrid_forward: table and out must be 8-byte aligned");
  const dim3 grid((R + HG_ROWS - 1) / HG_ROWS), block(RIGGS_WAVE * L);
  if (D == 3)
    hipLaunchKernelGGL(hashgrid_forward_kernel<3>, grid, block, 0, (hipStream_t)stream, k, L, (int)R, x, (const float2*)table, mask, (float2*)out);
  else
    hipLaunchKernelGGL(hashgrid_forward_kernel<4>, grid, block, 0, (hipStream_t)stream, k, L, (int)R, x, (const float2*)table, mask, (float2*)out);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_hashgrid_backward(const uint32_t* levels, int32_t R, const float* x, const float* mask, const float* g_out,
                            float* g_table, riggs_stream stream) {
  HgLevels k; const char* why; int D = 0, L = 0;
  RIGGS_REQUIRE(hg_check(levels, k, D, L, why) == 0, why);
  RIGGS_REQUIRE(R >= 0 && (int64_t)R * 2 * L < (1ll << 31), "riggs_hashgrid_backward: needs 0 <= R < 2^31 / (L F)");
  if (R == 0) return 0;
  RIGGS_REQUIRE(x && g_out && g_table, "riggs_hashgrid_backward: NULL argument");
  RIGGS_REQUIRE(hg_aligned8(g_out) && hg_aligned8(g_table), "riggs_hashgrid_backward: g_out and g_table must be 8-byte aligned");
  const dim3 grid((R + HG_ROWS - 1) / HG_ROWS), block(RIGGS_WAVE * L);
  if (D == 3)
    hipLaunchKernelGGL(hashgrid_backward_kernel<3>, grid, block, 0, (hipStream_t)stream, k, L, (int)R, x, mask, (const float2*)g_out, (float2*)g_table);
  else
    hipLaunchKernelGGL(hashgrid_backward_kernel<4>, grid, block, 0, (hipStream_t)stream, k, L, (int)R, x, mask, (const float2*)g_out, (float2*)g_table);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
