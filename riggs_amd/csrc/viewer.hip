// The editor's display step on the device (riggs_amd/viewer.py): interactive_GUI.py::test_step :497-664 and its overlay
// builders :97-247, render_rig.py::project_nodes_to_2d_withnodes :40-94, utils/other_utils.py::depth2normal :78-97.
//   viewer_range_*      min / max of a depth map, two fixed-order stages, no atomics (:614)
//   viewer_normal       depth2normal
//   viewer_project      points -> a table of overlay primitives (both projection rules of the reference)
//   viewer_compose      base colour by mode, bilinear resize, overlays in paint order: one launch, one 16 x 16 tile per workgroup
// Built with FP contraction off: every step rounds once, as the reference's separate torch kernels do.
//
// Coverage (include/riggs_hip.h states the rule): all operands are integers with |coordinate| <= RIGGS_VIEWER_COORD_MAX = 8192
// and a doubled extent e2 <= RIGGS_VIEWER_EXT2_MAX = 4096, so differences are <= 2^14, a cross product <= 2^29, 4 cross^2 <= 2^60
// and e2^2 |d|^2 <= 2^24 * 2^29: everything is exact in int64, here and in the NumPy restatement of the tests.
#include "common.h"

namespace riggs {

#define VW RIGGS_VIEWER_PRIM_WORDS
#define VIEWER_LIST_CAP 512   // LDS list entries; a chunk appends at most 256, so the list is walked once it holds more than 256
#define VIEWER_LIST_WORDS 10  // kind, x0, y0, x1, y1, colour e2, alpha e2, r, g, b

// ------------------------------------------------------------------------------------------------ depth range
// torch.min / torch.max: a NaN wins.
__device__ __forceinline__ float min_nan(float m, float v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

__device__ __forceinline__ void block_min_max(float& lo, float& hi, float* sh /* 8 floats */) {
  for (int o = 32; o > 0; o >>= 1) {
    lo = min_nan(lo, __shfl_xor(lo, o));
    hi = max_nan(hi, __shfl_xor(hi, o));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[wave] = lo; sh[4 + wave] = hi; }
  __syncthreads();
  lo = sh[0]; hi = sh[4];
#pragma unroll
  for (int v = 1; v < 4; v++) { lo = min_nan(lo, sh[v]); hi = max_nan(hi, sh[4 + v]); }
}

// stage 1: block b reduces the elements b * 256 + t, + gridDim * 256, ...: partial[2 b], partial[2 b + 1]
__global__ __launch_bounds__(256) void viewer_range_partial_kernel(long long n, const float* __restrict__ d, float* __restrict__ partial) {
  __shared__ float sh[8];
  float lo = d[0], hi = d[0];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = d[i];
    lo = min_nan(lo, v);
    hi = max_nan(hi, v);
  }
  block_min_max(lo, hi, sh);
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = lo; partial[2 * blockIdx.x + 1] = hi; }
}

// stage 2: one workgroup over the nb <= 256 partials
__global__ __launch_bounds__(256) void viewer_range_final_kernel(int nb, const float* __restrict__ partial, float* __restrict__ out) {
  __shared__ float sh[8];
  const int b = (int)threadIdx.x < nb ? (int)threadIdx.x : 0;
  float lo = partial[2 * b], hi = partial[2 * b + 1];
  block_min_max(lo, hi, sh);
  if (threadIdx.x == 0) { out[0] = lo; out[1] = hi; }
}

// ------------------------------------------------------------------------------------------------ depth2normal
// other_utils.py:85-96 at source pixel (y, x): replicate padding, the central differences -0.5 / +0.5, the division by
// depth + 1e-10, times focal, a 1 appended, normalised.
__device__ __forceinline__ void normal_at(const float* __restrict__ d, int h, int w, int y, int x, float focal, float n[3]) {
  const int xl = x > 0 ? x - 1 : 0, xr = x < w - 1 ? x + 1 : w - 1;
  const int yu = y > 0 ? y - 1 : 0, yd = y < h - 1 ? y + 1 : h - 1;
  const float* row = d + (size_t)y * w;
  const float gx = -0.5f * row[xl] + 0.5f * row[xr];
  const float gy = -0.5f * d[(size_t)yu * w + x] + 0.5f * d[(size_t)yd * w + x];
  const float den = row[x] + 1e-10f;
  const float nx = gx / den * focal, ny = gy / den * focal;
  const float norm = sqrtf((nx * nx + ny * ny) + 1.0f);
  n[0] = nx / norm; n[1] = ny / norm; n[2] = 1.0f / norm;
}

__global__ __launch_bounds__(256) void viewer_normal_kernel(int h, int w, const float* __restrict__ d, float focal, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= hw) return;
  float n[3];
  normal_at(d, h, w, (int)(i / w), (int)(i % w), focal, n);
  out[i] = n[0]; out[hw + i] = n[1]; out[2 * hw + i] = n[2];
}

// ------------------------------------------------------------------------------------------------ projection
struct Projected { float u, v; bool ok; };

// Editor rule (interactive_GUI.py:141-143, :166-168, :226-228): uv = (p_hom @ full_proj)[:2] / w, then (uv + 1) / 2 * [image_height,
// image_width] — x IS SCALED BY THE HEIGHT and y by the width, as the reference writes it (the two agree on its square windows).
// render_rig rule (render_rig.py:59-62): fx x / z + cx + 0.5, fy y / z + cy + 0.5 in camera space.
// ok: every coordinate finite and w (or z) > 0.
__device__ __forceinline__ Projected project_point(const riggs_viewer_projection& a, const float* __restrict__ p) {
  const float* M = a.matrix;
  const float x = p[0], y = p[1], z = p[2];
  Projected r;
  if (a.rule == RIGGS_VIEWER_RULE_EDITOR) {
    const float X = ((x * M[0] + y * M[4]) + z * M[8]) + M[12];
    const float Y = ((x * M[1] + y * M[5]) + z * M[9]) + M[13];
    const float Wc = ((x * M[3] + y * M[7]) + z * M[11]) + M[15];
    r.u = (X / Wc + 1.0f) / 2.0f * a.scale_x;
    r.v = (Y / Wc + 1.0f) / 2.0f * a.scale_y;
    r.ok = Wc > 0.0f;
  } else {
    const float X = ((x * M[0] + y * M[4]) + z * M[8]) + M[12];
    const float Y = ((x * M[1] + y * M[5]) + z * M[9]) + M[13];
    const float Z = ((x * M[2] + y * M[6]) + z * M[10]) + M[14];
    r.u = (a.fx * X / Z + a.cx) + 0.5f;
    r.v = (a.fy * Y / Z + a.cy) + 0.5f;
    r.ok = Z > 0.0f;
  }
  r.ok = r.ok && isfinite(r.u) && isfinite(r.v);
  return r;
}

// astype(np.int32) / .int(): toward zero; then the coordinate clamp (the two commute: the bounds are integers)
__device__ __forceinline__ int to_pixel(float v) {
  const float lim = (float)RIGGS_VIEWER_COORD_MAX;
  return (int)fminf(fmaxf(v, -lim), lim);
}

__device__ __forceinline__ void write_prim(int* __restrict__ rec, int kind, int x0, int y0, int x1, int y1, int ec, int ea,
                                           float r, float g, float b, bool ok) {
  rec[0] = kind; rec[1] = x0; rec[2] = y0; rec[3] = x1; rec[4] = y1; rec[5] = ec; rec[6] = ea;
  rec[7] = __float_as_int(r); rec[8] = __float_as_int(g); rec[9] = __float_as_int(b);
  rec[10] = ok ? 1 : 0; rec[11] = 0;
}

// one thread per primitive; the (at most two) points of a primitive are projected by its own thread
__global__ __launch_bounds__(256) void viewer_project_kernel(riggs_viewer_projection a, int P) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  int* rec = a.table ? a.table + (size_t)p * VW : nullptr;
  if (a.layout == RIGGS_VIEWER_LAYOUT_SKELETON) {
    // edges i = 1 .. n-1 (joint i -> its parent), discs i = 0 .. n-1; the reference skeleton paints its discs first
    const int n = a.n, ne = n - 1;
    const bool is_edge = a.discs_first ? p >= n : p < ne;
    const int i = a.discs_first ? (is_edge ? p - n + 1 : p) : (is_edge ? p + 1 : p - ne);
    const Projected q = project_point(a, a.points + 3 * (size_t)i);
    if (is_edge) {
      int par = a.parents[i];
      par = par < 0 ? 0 : (par >= n ? n - 1 : par);
      const Projected o = project_point(a, a.points + 3 * (size_t)par);
      if (rec) write_prim(rec, RIGGS_VIEWER_SEGMENT, to_pixel(q.u), to_pixel(q.v), to_pixel(o.u), to_pixel(o.v), a.segment_ext2, a.segment_ext2,
                          a.rgb[0], a.rgb[1], a.rgb[2], q.ok && o.ok);
    } else {
      const float* c = a.colors ? a.colors + 3 * (size_t)i : a.rgb + 3;
      if (rec) write_prim(rec, RIGGS_VIEWER_DISC, to_pixel(q.u), to_pixel(q.v), to_pixel(q.u), to_pixel(q.v), a.disc_color_ext2, a.disc_alpha_ext2,
                          c[0], c[1], c[2], q.ok);
      if (a.uv) { a.uv[2 * i] = q.u; a.uv[2 * i + 1] = q.v; }
    }
  } else if (a.layout == RIGGS_VIEWER_LAYOUT_SQUARES) {
    // :119-121 left_top = uv - r, right_bottom = uv + r, each truncated on its own
    const Projected q = project_point(a, a.points + 3 * (size_t)p);
    const float r = (float)a.square_radius;
    const float* c = a.colors ? a.colors + 3 * (size_t)p : a.rgb;
    if (rec) write_prim(rec, RIGGS_VIEWER_SQUARE, to_pixel(q.u - r), to_pixel(q.v - r), to_pixel(q.u + r), to_pixel(q.v + r), 0, 0, c[0], c[1], c[2], q.ok);
    if (a.uv) { a.uv[2 * p] = q.u; a.uv[2 * p + 1] = q.v; }
  } else {
    // polylines: track g = p / (S - 1), its samples s and s + 1 of a ring of `ring_capacity` slots (n, 3) whose oldest is `ring_head`
    const int segs = a.samples - 1;
    const int g = p / segs, s = p % segs;
    const int s0 = (a.ring_head + s) % a.ring_capacity, s1 = (a.ring_head + s + 1) % a.ring_capacity;
    const Projected q = project_point(a, a.points + 3 * ((size_t)s0 * a.n + g));
    const Projected o = project_point(a, a.points + 3 * ((size_t)s1 * a.n + g));
    const float* c = a.colors ? a.colors + 3 * (size_t)g : a.rgb;
    if (rec) write_prim(rec, RIGGS_VIEWER_SEGMENT, to_pixel(q.u), to_pixel(q.v), to_pixel(o.u), to_pixel(o.v), a.segment_ext2, a.segment_ext2,
                        c[0], c[1], c[2], q.ok && o.ok);
  }
}

// ------------------------------------------------------------------------------------------------ compose
// Is pixel (px, py) inside the colour shape / the alpha shape of a primitive?  num <= e2^2 den with (num, den) = (4 d^2, 1) for
// a point distance (discs, the round caps, zero-length segments) and (4 cross^2, |d|^2) for the body of a segment.
__device__ __forceinline__ void covered(const int* __restrict__ e, int px, int py, bool& in_c, bool& in_a) {
  const int kind = e[0];
  const long long x0 = e[1], y0 = e[2], x1 = e[3], y1 = e[4];
  if (kind == RIGGS_VIEWER_SQUARE) {
    in_c = in_a = px >= x0 && px <= x1 && py >= y0 && py <= y1;
    return;
  }
  const long long ex = px - x0, ey = py - y0;
  long long num = 4 * (ex * ex + ey * ey), den = 1;
  if (kind == RIGGS_VIEWER_SEGMENT) {
    const long long dx = x1 - x0, dy = y1 - y0;
    const long long l2 = dx * dx + dy * dy, t = ex * dx + ey * dy;
    if (l2 > 0 && t > 0) {
      if (t >= l2) {
        const long long fx = px - x1, fy = py - y1;
        num = 4 * (fx * fx + fy * fy);
      } else {
        const long long c = ex * dy - ey * dx;
        num = 4 * c * c;
        den = l2;
      }
    }
  }
  const long long ec = e[5], ea = e[6];
  in_c = num <= ec * ec * den;
  in_a = num <= ea * ea * den;
}

struct Paint { float r, g, b, a; };

__device__ __forceinline__ void walk_list(const int* __restrict__ list, int count, int px, int py, Paint& s) {
  for (int i = 0; i < count; i++) {
    const int* e = list + i * VIEWER_LIST_WORDS;  // (every lane reads the same words: LDS broadcasts)
    bool in_c, in_a;
    covered(e, px, py, in_c, in_a);
    if (in_c) { s.r = __int_as_float(e[7]); s.g = __int_as_float(e[8]); s.b = __int_as_float(e[9]); }
    if (in_a) s.a = 1.0f;
  }
}

// ATen's upsample_bilinear2d source index for align_corners=False: scale * (dst + 0.5) - 0.5, negative -> 0
__device__ __forceinline__ void bilinear_tap(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  i0 = (int)src;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.0f - l1;
}

__device__ __forceinline__ void base_at(const riggs_viewer_frame& f, int y, int x, float lo, float hi, float c[3]) {
  const size_t hw = (size_t)f.src_height * f.src_width, i = (size_t)y * f.src_width + x;
  if (f.mode == RIGGS_VIEWER_MODE_IMAGE) {
    c[0] = f.source[i]; c[1] = f.source[hw + i]; c[2] = f.source[2 * hw + i];
  } else if (f.mode == RIGGS_VIEWER_MODE_DEPTH) {  // :612-614
    c[0] = c[1] = c[2] = (f.source[i] - lo) / ((hi - lo) + 1e-20f);
  } else if (f.mode == RIGGS_VIEWER_MODE_ALPHA) {
    c[0] = c[1] = c[2] = f.source[i];
  } else {  // :523-524, evaluated at the source pixel a tap reads
    float n[3];
    normal_at(f.source, f.src_height, f.src_width, y, x, f.focal, n);
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = (n[k] + 1.0f) / 2.0f;
  }
}

__global__ __launch_bounds__(256) void viewer_compose_kernel(riggs_viewer_frame f) {
  __shared__ int list[VIEWER_LIST_CAP * VIEWER_LIST_WORDS];
  __shared__ int wave_count[4];
  __shared__ float tile_rgb[RIGGS_TILE * RIGGS_TILE * 3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tx0 = blockIdx.x * RIGGS_TILE, ty0 = blockIdx.y * RIGGS_TILE;
  const int px = tx0 + (t & 15), py = ty0 + (t >> 4);
  const bool in_window = px < f.width && py < f.height;

  // ---- base colour: mode, bilinear resize, clamp
  float base[3] = {0.0f, 0.0f, 0.0f};
  if (in_window) {
    float lo = 0.0f, hi = 0.0f;
    if (f.mode == RIGGS_VIEWER_MODE_DEPTH) { lo = f.range[0]; hi = f.range[1]; }
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    bilinear_tap(f.scale_h, py, f.src_height, y0, y1, hy0, hy1);
    bilinear_tap(f.scale_w, px, f.src_width, x0, x1, wx0, wx1);
    float c00[3], c01[3], c10[3], c11[3];
    base_at(f, y0, x0, lo, hi, c00);
    base_at(f, y0, x1, lo, hi, c01);
    base_at(f, y1, x0, lo, hi, c10);
    base_at(f, y1, x1, lo, hi, c11);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float v = hy0 * (wx0 * c00[k] + wx1 * c01[k]) + hy1 * (wx0 * c10[k] + wx1 * c11[k]);
      base[k] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
  }

  // ---- overlays: one group per table, blended one after another (:641-654)
  for (int g = 0; g < f.num_tables; g++) {
    const int* __restrict__ table = f.tables[g];
    const int P = f.counts[g];
    Paint s = {0.0f, 0.0f, 0.0f, 0.0f};
    int count = 0;  // entries of the LDS list; the same in every thread
    for (int first = 0; first < P; first += 256) {
      if (count > VIEWER_LIST_CAP - 256) {  // the list may not take another chunk: paint what it holds, in order, and go on
        walk_list(list, count, px, py, s);
        count = 0;
      }
      // each thread tests one primitive's bounding box, grown by its extent, against the tile
      const int p = first + t;
      bool keep = false;
      const int* rec = table + (size_t)(p < P ? p : 0) * VW;
      int kind = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0, ec = 0, ea = 0;
      if (p < P && rec[10] != 0) {
        kind = rec[0]; x0 = rec[1]; y0 = rec[2]; x1 = rec[3]; y1 = rec[4]; ec = rec[5]; ea = rec[6];
        const int grow = kind == RIGGS_VIEWER_SQUARE ? 0 : ((ec > ea ? ec : ea) + 1) / 2;
        const int bx0 = (x0 < x1 ? x0 : x1) - grow, bx1 = (x0 > x1 ? x0 : x1) + grow;
        const int by0 = (y0 < y1 ? y0 : y1) - grow, by1 = (y0 > y1 ? y0 : y1) + grow;
        keep = bx0 <= tx0 + RIGGS_TILE - 1 && bx1 >= tx0 && by0 <= ty0 + RIGGS_TILE - 1 && by1 >= ty0;
      }
      // survivors are compacted in table order: ballot + prefix popcount per wave, the waves' offsets through LDS
      const unsigned long long mask = __ballot(keep);
      if (lane == 0) wave_count[wave] = __popcll(mask);
      __syncthreads();  // (also: every thread has finished walking the list before anyone appends to it)
      int offset = count, total = 0;
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int c = wave_count[v];
        if (v < wave) offset += c;
        total += c;
      }
      if (keep) {
        int* e = list + (offset + __popcll(mask & ((1ull << lane) - 1ull))) * VIEWER_LIST_WORDS;
        e[0] = kind; e[1] = x0; e[2] = y0; e[3] = x1; e[4] = y1; e[5] = ec; e[6] = ea; e[7] = rec[7]; e[8] = rec[8]; e[9] = rec[9];
      }
      count += total;
      __syncthreads();
    }
    walk_list(list, count, px, py, s);
    if (f.rules[g] == RIGGS_VIEWER_BLEND_ALPHA) {  // out = base (1 - a) + rgb a over the two painted layers
      base[0] = base[0] * (1.0f - s.a) + s.r * s.a;
      base[1] = base[1] * (1.0f - s.a) + s.g * s.a;
      base[2] = base[2] * (1.0f - s.a) + s.b * s.a;
    } else {  // :651-654 base * (sum(overlay) == 0) + overlay
      const float m = ((s.r + s.g) + s.b) == 0.0f ? 1.0f : 0.0f;
      base[0] = base[0] * m + s.r;
      base[1] = base[1] * m + s.g;
      base[2] = base[2] * m + s.b;
    }
    __syncthreads();  // the next group's chunks overwrite the list
  }

  // ---- HWC output: the tile's 16 rows of 48 floats, each written as one contiguous run
  tile_rgb[3 * t] = base[0]; tile_rgb[3 * t + 1] = base[1]; tile_rgb[3 * t + 2] = base[2];
  __syncthreads();
  const int cols = (f.width - tx0 < RIGGS_TILE ? f.width - tx0 : RIGGS_TILE) * 3;
  for (int i = t; i < RIGGS_TILE * RIGGS_TILE * 3; i += 256) {
    const int row = i / (RIGGS_TILE * 3), col = i % (RIGGS_TILE * 3);
    if (ty0 + row < f.height && col < cols) f.out[((size_t)(ty0 + row) * f.width + tx0) * 3 + col] = tile_rgb[i];
  }
}

}  // namespace riggs

using namespace riggs;

extern "C" int riggs_viewer_depth_range(int64_t n, const float* depth, float* workspace, float* out_min_max, riggs_stream stream) {
  RIGGS_REQUIRE(n >= 1, "riggs_viewer_depth_range: the depth map is empty");
  RIGGS_REQUIRE(depth && workspace && out_min_max, "riggs_viewer_depth_range: NULL buffer");
  const long long per_block = 256 * 8;
  long long nb = (n + per_block - 1) / per_block;
  nb = nb > RIGGS_VIEWER_RANGE_WORKSPACE_FLOATS / 2 ? RIGGS_VIEWER_RANGE_WORKSPACE_FLOATS / 2 : nb;
  hipLaunchKernelGGL(viewer_range_partial_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (long long)n, depth, workspace);
  hipLaunchKernelGGL(viewer_range_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (int)nb, (const float*)workspace, out_min_max);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int riggs_viewer_depth2normal(int32_t h, int32_t w, const float* depth, float focal, float* out, riggs_stream stream) {
  RIGGS_REQUIRE(h >= 1 && w >= 1, "riggs_viewer_depth2normal: bad shape");
  RIGGS_REQUIRE(depth && out, "riggs_viewer_depth2normal: NULL buffer");
  const long long hw = (long long)h * w;
  RIGGS_REQUIRE((hw + 255) / 256 <= 0x7fffffffLL, "riggs_viewer_depth2normal: the depth map is too large");
  hipLaunchKernelGGL(viewer_normal_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h, w, depth, focal, out);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int64_t riggs_viewer_project_count(const riggs_viewer_projection* p) {
  if (!p || p->n < 0) return -1;
  switch (p->layout) {
    case RIGGS_VIEWER_LAYOUT_SKELETON: return p->n == 0 ? 0 : 2 * (int64_t)p->n - 1;
    case RIGGS_VIEWER_LAYOUT_SQUARES: return p->n;
    case RIGGS_VIEWER_LAYOUT_POLYLINES: return p->samples < 2 ? 0 : (int64_t)p->n * (p->samples - 1);
    default: return -1;
  }
}

extern "C" int riggs_viewer_project(const riggs_viewer_projection* p, riggs_stream stream) {
  RIGGS_REQUIRE(p, "riggs_viewer_project: NULL projection");
  const int64_t P = riggs_viewer_project_count(p);
  RIGGS_REQUIRE(P >= 0, "riggs_viewer_project: unknown layout or a negative count");
  RIGGS_REQUIRE(p->rule == RIGGS_VIEWER_RULE_EDITOR || p->rule == RIGGS_VIEWER_RULE_RENDER_RIG, "riggs_viewer_project: unknown rule");
  RIGGS_REQUIRE(P <= (int64_t)1 << 24, "riggs_viewer_project: more than 2^24 primitives");
  if (P == 0) return 0;
  RIGGS_REQUIRE(p->points && p->matrix && (p->table || p->uv), "riggs_viewer_project: NULL buffer");
  RIGGS_REQUIRE(p->layout != RIGGS_VIEWER_LAYOUT_SKELETON || p->parents, "riggs_viewer_project: the skeleton layout needs parents");
  RIGGS_REQUIRE(p->layout != RIGGS_VIEWER_LAYOUT_POLYLINES ||
                    (p->ring_capacity >= p->samples && p->ring_head >= 0 && p->ring_head < p->ring_capacity && !p->uv),
                "riggs_viewer_project: bad ring (samples <= ring_capacity, 0 <= ring_head < ring_capacity, no uv)");
  RIGGS_REQUIRE(p->segment_ext2 >= 0 && p->segment_ext2 <= RIGGS_VIEWER_EXT2_MAX && p->disc_color_ext2 >= 0 &&
                    p->disc_color_ext2 <= RIGGS_VIEWER_EXT2_MAX && p->disc_alpha_ext2 >= 0 && p->disc_alpha_ext2 <= RIGGS_VIEWER_EXT2_MAX &&
                    p->square_radius >= 0 && p->square_radius <= RIGGS_VIEWER_EXT2_MAX,
                "riggs_viewer_project: an extent outside 0 .. RIGGS_VIEWER_EXT2_MAX");
  hipLaunchKernelGGL(viewer_project_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *p, (int)P);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int riggs_viewer_compose(const riggs_viewer_frame* f, riggs_stream stream) {
  RIGGS_REQUIRE(f, "riggs_viewer_compose: NULL frame");
  RIGGS_REQUIRE(f->mode >= RIGGS_VIEWER_MODE_IMAGE && f->mode <= RIGGS_VIEWER_MODE_NORMAL, "riggs_viewer_compose: unknown mode");
  RIGGS_REQUIRE(f->src_height >= 1 && f->src_width >= 1 && f->height >= 1 && f->width >= 1, "riggs_viewer_compose: bad shape");
  RIGGS_REQUIRE(f->height <= RIGGS_VIEWER_COORD_MAX && f->width <= RIGGS_VIEWER_COORD_MAX,
                "riggs_viewer_compose: the window is larger than RIGGS_VIEWER_COORD_MAX on a side");
  RIGGS_REQUIRE(f->source && f->out, "riggs_viewer_compose: NULL buffer");
  RIGGS_REQUIRE(f->mode != RIGGS_VIEWER_MODE_DEPTH || f->range, "riggs_viewer_compose: the depth mode needs the range");
  RIGGS_REQUIRE(f->num_tables >= 0 && f->num_tables <= RIGGS_VIEWER_MAX_TABLES, "riggs_viewer_compose: too many tables");
  for (int g = 0; g < f->num_tables; g++) {
    RIGGS_REQUIRE(f->counts[g] >= 0 && (f->counts[g] == 0 || f->tables[g]), "riggs_viewer_compose: a table is NULL or has a negative count");
    RIGGS_REQUIRE(f->rules[g] == RIGGS_VIEWER_BLEND_ALPHA || f->rules[g] == RIGGS_VIEWER_BLEND_MASK, "riggs_viewer_compose: unknown blend rule");
  }
  const dim3 grid((unsigned)((f->width + RIGGS_TILE - 1) / RIGGS_TILE), (unsigned)((f->height + RIGGS_TILE - 1) / RIGGS_TILE));
  hipLaunchKernelGGL(viewer_compose_kernel, grid, dim3(256), 0, (hipStream_t)stream, *f);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}
