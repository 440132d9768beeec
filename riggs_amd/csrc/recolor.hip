// Compositing a second colour set over the tile lists of a frame that has already been rendered (include/riggs_hip.h:
// riggs_raster_recolor_forward / _backward).
//
// A frame's arenas hold everything a second image of the SAME geometry needs: the sorted instance list, the tile ranges, the
// screen-space records (centre, conic, opacity), and per pixel the final transmittance and the list position behind its last
// contributor (n_contrib).  Nothing is projected, sorted or binned again: a 16 x 16 tile is one 256-thread workgroup, a lane is a
// pixel, the tile's list is staged through LDS 256 instances at a time and walked front to back up to the workgroup's largest
// n_contrib — exactly the instances the frame's own forward composited, so no transmittance stop test is needed.
// The backward is the colour gradient only (dL/dc_n = sum over pixels of alpha T dL/dpixel): the same walk with the running
// transmittance, no back-to-front reconstruction; per (instance, tile) the three partial sums are folded across the wave by
// DPP, across the four waves through LDS in wave order, and leave as one float-atomic triple.
// Every arena is read only: the frame's own backward still finds what its forward left.
#include "raster_internal.h"

namespace riggs {

// the alpha evaluation of render_bwd_kernel (render.hip) on the geometry arena: the same constants (raster_internal.h), the same
// expression order, the same tests

struct RecolorArgs {
  int W, H, N;
  int64_t cap;
  const uint2* ranges;
  const uint32_t* point_list;
  const float4 *xyd, *conic_o;
  const float* final_T;
  const uint32_t* n_contrib;
  const uint32_t* counters;  // the frame's {R, overflow flag, ..} or NULL (no guard)
  const float* colors;       // (N, 3): forward
  const float* bg;           // (3,): forward
  float* out_color;          // (3, H, W): forward
  const float* dL_dcolor;    // (3, H, W): backward
  float* dL_dcolors;         // (N, 3): backward; zero on entry
};

#define RC_ROUND 256

// alpha of the staged instance at this lane's pixel, or 0 when it does not contribute (power > 0, alpha < 1/255)
__device__ __forceinline__ float rc_alpha(const float2 xy, const float4 co, const float pfx, const float pfy) {
  const float dx = xy.x - pfx, dy = xy.y - pfy;
  const float cyy = co.z * dy * dy, cody = co.y * dy;
  const float pw = -0.5f * (co.x * dx * dx + cyy) - cody * dx;
  const float al = fminf(ALPHA_MAX, co.w * fast_exp(pw));
  return ((pw <= 0.0f) && (al >= ALPHA_MIN)) ? al : 0.f;
}

__device__ __forceinline__ uint32_t rc_wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// what a workgroup knows about its tile before the walk
struct RcTile {
  uint32_t start;   // first list position of the tile
  uint32_t n;       // this lane's pixel: instances of the tile's list in front of and including its last contributor (0: none / outside)
  uint32_t n_wave;  // largest n of this wave's pixels
  uint32_t n_max;   // largest n of the tile
  bool inside;
  size_t pid;
  float pfx, pfy;
};
__device__ __forceinline__ RcTile rc_tile(const RecolorArgs& a, uint32_t* s_max) {
  RcTile t;
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int gx = (a.W + RIGGS_TILE - 1) / RIGGS_TILE;
  const int pxi = (tile % gx) * RIGGS_TILE + (tid & 15), pyi = (tile / gx) * RIGGS_TILE + (tid >> 4);
  t.inside = pxi < a.W && pyi < a.H;
  t.pid = (size_t)pyi * a.W + pxi;
  t.pfx = (float)pxi; t.pfy = (float)pyi;
  const uint2 rg = a.ranges[tile];
  // (an overflowed frame — unguarded call — has ranges beyond the arena: the walk stays inside it)
  const uint64_t end = (uint64_t)rg.y < (uint64_t)a.cap ? (uint64_t)rg.y : (uint64_t)a.cap;
  const uint32_t len = (a.N > 0 && end > (uint64_t)rg.x) ? (uint32_t)(end - rg.x) : 0u;
  t.start = rg.x;
  t.n = t.inside ? min(a.n_contrib[t.pid], len) : 0u;
  t.n_wave = rc_wave_max(t.n);
  if ((tid & 63) == 0) s_max[tid >> 6] = t.n_wave;
  __syncthreads();
  t.n_max = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
  return t;
}

__global__ __launch_bounds__(256) void recolor_fwd_kernel(RecolorArgs a) {
  __shared__ float2 s_xy[RC_ROUND];
  __shared__ float4 s_co[RC_ROUND];
  __shared__ float4 s_c[RC_ROUND];
  __shared__ uint32_t s_max[4];
  const int tid = threadIdx.x;
  const size_t HW = (size_t)a.H * a.W;
  const bool overflowed = a.counters != nullptr && a.counters[1] != 0u;  // the frame composited truncated lists: a zero image
  RcTile t = rc_tile(a, s_max);
  if (overflowed) {
    if (t.inside) { a.out_color[t.pid] = 0.f; a.out_color[HW + t.pid] = 0.f; a.out_color[2 * HW + t.pid] = 0.f; }
    return;
  }
  float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f;
  for (uint32_t base = 0; base < t.n_max; base += RC_ROUND) {
    const uint32_t pos = base + tid;
    if (pos < t.n_max) {
      uint32_t id = a.point_list[(size_t)t.start + pos];
      id = id < (uint32_t)a.N ? id : 0u;
      const float4 xy = a.xyd[id];
      s_xy[tid] = make_float2(xy.x, xy.y);
      s_co[tid] = a.conic_o[id];
      const float* c = a.colors + (size_t)id * 3;
      s_c[tid] = make_float4(c[0], c[1], c[2], 0.f);
    }
    __syncthreads();
    // (wave-uniform bound: this wave's pixels have no contributor behind n_wave)
    const int cnt = t.n_wave > base ? (int)min(t.n_wave - base, (uint32_t)RC_ROUND) : 0;
    for (int j = 0; j < cnt; j++) {
      float al = rc_alpha(s_xy[j], s_co[j], t.pfx, t.pfy);
      al = (base + j < t.n) ? al : 0.f;
      const float4 c = s_c[j];
      const float w = al * T;
      C0 += c.x * w; C1 += c.y * w; C2 += c.z * w;
      T *= 1.0f - al;
    }
    __syncthreads();
  }
  if (t.inside) {
    const float Tf = a.final_T[t.pid];
    a.out_color[t.pid] = C0 + Tf * a.bg[0];
    a.out_color[HW + t.pid] = C1 + Tf * a.bg[1];
    a.out_color[2 * HW + t.pid] = C2 + Tf * a.bg[2];
  }
}

__global__ __launch_bounds__(256) void recolor_bwd_kernel(RecolorArgs a) {
  __shared__ float2 s_xy[RC_ROUND];
  __shared__ float4 s_co[RC_ROUND];
  __shared__ float s_part[4][RC_ROUND][3];  // per wave and staged instance: the wave's partial sums (zero: the wave skipped it)
  __shared__ uint32_t s_max[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t HW = (size_t)a.H * a.W;
  if (a.counters != nullptr && a.counters[1] != 0u) return;  // an overflowed frame: the gradient stays the zeros it was filled with
  RcTile t = rc_tile(a, s_max);
  float g0 = 0.f, g1 = 0.f, g2 = 0.f;
  if (t.n > 0u) { g0 = a.dL_dcolor[t.pid]; g1 = a.dL_dcolor[HW + t.pid]; g2 = a.dL_dcolor[2 * HW + t.pid]; }
  float T = 1.0f;
  for (uint32_t base = 0; base < t.n_max; base += RC_ROUND) {
    const uint32_t pos = base + tid;
    uint32_t id = 0u;
    if (pos < t.n_max) {
      id = a.point_list[(size_t)t.start + pos];
      id = id < (uint32_t)a.N ? id : 0u;
      const float4 xy = a.xyd[id];
      s_xy[tid] = make_float2(xy.x, xy.y);
      s_co[tid] = a.conic_o[id];
    }
#pragma unroll
    for (int w = 0; w < 4; w++) { s_part[w][tid][0] = 0.f; s_part[w][tid][1] = 0.f; s_part[w][tid][2] = 0.f; }
    __syncthreads();
    const int cnt = t.n_wave > base ? (int)min(t.n_wave - base, (uint32_t)RC_ROUND) : 0;
    for (int j = 0; j < cnt; j++) {
      float al = rc_alpha(s_xy[j], s_co[j], t.pfx, t.pfy);
      al = (base + j < t.n) ? al : 0.f;
      const float w = al * T;
      T *= 1.0f - al;
      if (__builtin_amdgcn_ballot_w64(w != 0.f) == 0) continue;  // no pixel of this wave sees the instance
      const float r0 = wave_sum(w * g0), r1 = wave_sum(w * g1), r2 = wave_sum(w * g2);
      if (lane == 63) { s_part[wave][j][0] = r0; s_part[wave][j][1] = r1; s_part[wave][j][2] = r2; }
    }
    __syncthreads();
    // one float-atomic triple per (instance, tile): lane <-> staged instance, the four waves' parts added in wave order
    if (pos < t.n_max) {
      const float r0 = ((s_part[0][tid][0] + s_part[1][tid][0]) + s_part[2][tid][0]) + s_part[3][tid][0];
      const float r1 = ((s_part[0][tid][1] + s_part[1][tid][1]) + s_part[2][tid][1]) + s_part[3][tid][1];
      const float r2 = ((s_part[0][tid][2] + s_part[1][tid][2]) + s_part[2][tid][2]) + s_part[3][tid][2];
      if (r0 != 0.f || r1 != 0.f || r2 != 0.f) {
        float* g = a.dL_dcolors + (size_t)id * 3;
        atomicAdd(g + 0, r0); atomicAdd(g + 1, r1); atomicAdd(g + 2, r2);
      }
    }
    // (the next round's staging rewrites s_part[.][tid] — this thread's own entries — and the records every wave has finished with)
  }
}

static int fill_recolor_args(RecolorArgs& a, const riggs_raster_cfg* cfg, const void* geom_, const void* binning_, int64_t cap,
                             const void* image_, const uint32_t* counters) {
  RIGGS_REQUIRE(cfg != nullptr, "cfg is NULL");
  const int N = cfg->num_points, H = cfg->image_height, W = cfg->image_width;
  RIGGS_REQUIRE(N >= 0 && H > 0 && W > 0, "bad sizes");
  RIGGS_REQUIRE(cap >= 0, "bad instance capacity");
  RIGGS_REQUIRE(image_ != nullptr, "image_state is NULL");
  RIGGS_REQUIRE(N == 0 || (geom_ != nullptr && binning_ != nullptr), "geom / binning is NULL");
  const char* geom = (const char*)geom_;
  const char* bin = (const char*)binning_;
  const char* img = (const char*)image_;
  const GeomLayout G = geom_layout(N);
  const ImageLayout I = image_layout(H, W);
  const BinLayout B = bin_layout(cap, N, H, W);
  memset(&a, 0, sizeof(a));
  a.W = W; a.H = H; a.N = N; a.cap = cap;
  a.ranges = (const uint2*)(img + I.ranges);
  a.point_list = (const uint32_t*)(bin + B.point_list);
  a.xyd = (const float4*)(geom + G.xyd); a.conic_o = (const float4*)(geom + G.conic_o);
  a.final_T = (const float*)(img + I.final_T); a.n_contrib = (const uint32_t*)(img + I.n_contrib);
  a.counters = counters;
  return 0;
}

static inline int recolor_tiles(const RecolorArgs& a) {
  return ((a.W + RIGGS_TILE - 1) / RIGGS_TILE) * ((a.H + RIGGS_TILE - 1) / RIGGS_TILE);
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_raster_recolor_forward(const riggs_raster_cfg* cfg, const void* geom, const void* binning, int64_t instance_capacity,
                                 const void* image_state, const uint32_t* counters, const float* colors, const float* bg,
                                 float* out_color, riggs_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  RecolorArgs a;
  const int rc = fill_recolor_args(a, cfg, geom, binning, instance_capacity, image_state, counters);
  if (rc) return rc;
  RIGGS_REQUIRE(bg != nullptr && out_color != nullptr, "bg / out_color is NULL");
  RIGGS_REQUIRE(a.N == 0 || colors != nullptr, "colors is NULL");
  a.colors = colors; a.bg = bg; a.out_color = out_color;
  // (N = 0: every range is empty and the frame's final transmittance is 1 — the image is bg)
  hipLaunchKernelGGL(recolor_fwd_kernel, dim3(recolor_tiles(a)), dim3(256), 0, s, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  if (debug_sync(cfg->debug, s, "recolor_fwd")) return 1;
  return 0;
}

int riggs_raster_recolor_backward(const riggs_raster_cfg* cfg, const void* geom, const void* binning, int64_t instance_capacity,
                                  const void* image_state, const uint32_t* counters, const float* dL_dcolor, float* dL_dcolors,
                                  riggs_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  RecolorArgs a;
  const int rc = fill_recolor_args(a, cfg, geom, binning, instance_capacity, image_state, counters);
  if (rc) return rc;
  if (a.N == 0) return 0;
  RIGGS_REQUIRE(dL_dcolor != nullptr && dL_dcolors != nullptr, "dL_dcolor / dL_dcolors is NULL");
  a.dL_dcolor = dL_dcolor; a.dL_dcolors = dL_dcolors;
  RIGGS_HIP_CHECK(hipMemsetAsync(dL_dcolors, 0, (size_t)a.N * 3 * sizeof(float), s));
  hipLaunchKernelGGL(recolor_bwd_kernel, dim3(recolor_tiles(a)), dim3(256), 0, s, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  if (debug_sync(cfg->debug, s, "recolor_bwd")) return 1;
  return 0;
}

}  // extern "C"
