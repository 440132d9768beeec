// 2-D skeleton thinning of silhouette masks: Guo and Hall's two-subiteration parallel thinning, the algorithm behind
// skimage.morphology.thin, which process_data/cal_2d_skeleton.py of the reference runs offline to make `train_thinned/*.png`
// (viewpoint_cam.thinned, the pixel set of csrc/skel_loss.hip).  Restated from the published algorithm, not from skimage's
// source; tests/thin_ref.py is the NumPy restatement these kernels are held to bit for bit.  Integer only.
//
// Neighbours of (r, c): x0 E, x1 NE, x2 N, x3 NW, x4 W, x5 SW, x6 S, x7 SE; outside the image they are 0.  A set pixel is deleted
// by a sub-iteration when, on the state before it,
//   G1  exactly one i in {0, 2, 4, 6} has x_i = 0 and (x_{i+1} or x_{i+2}),
//   G2  min(n1, n2) in {2, 3}, n1 = sum_{k odd} (x_k or x_{k-1}), n2 = sum_{k odd} (x_k or x_{k+1}),
//   G3  not ((x1 or x2 or not x7) and x0) in the first sub-iteration, the same under a 180 degree turn of the neighbourhood
//       (x_i -> x_{i+4}) in the second: not ((x5 or x6 or not x3) and x4).  G1 and G2 are invariant under that turn.
//
// BIT PLANE.  One bit per pixel, bit k of word j of a row is column 32 j + k; Wd = ceil(W / 32) words per row, the bits past W
// are 0 and stay 0 (thinning never sets a pixel).  A plane is stored PADDED: rows -1 .. H of S = Wd + 1 words each behind one
// leading word, (H + 2) S + 1 words, every pad word 0.  Word j of row r sits at 1 + (r + 1) S + j; its left and right
// neighbours are the words before and after it (the pad word that ends a row is also what precedes the next row's word 0) and
// the rows above and below are S words away, so the eight neighbour words of any interior word are read without a bounds test
// and the image border reads 0.  thin_word() decides 32 pixels at once from those nine words by bit-parallel boolean logic.
//
// LDS PATH (thin_lds_kernel): one 1024-lane workgroup per image, grid = batch.  The padded plane lives in dynamic LDS for the
// whole run (up to the 160 KiB one workgroup may claim on gfx950: riggs_thin_path says whether an image fits); every lane owns
// the words i = k 1024 + lane, k < 40, of the sweep and keeps them in registers, so LDS serves the neighbours only.  A
// sub-iteration: new words from registers + LDS, barrier, changed words to LDS, barrier.  After every second sub-iteration the
// workgroup stops if the pair deleted nothing.  No host synchronisation; the images of a batch converge independently.
//
// GLOBAL PATH: the same thin_word over padded planes ping-ponged in the caller's workspace, one launch per sub-iteration over
// the batch; the last pair of every `check_every` iterations counts its deletions per image on the device and the host reads
// the counters back (this path synchronises the stream).  A fixed point is idempotent, so the iterations a converged image
// runs until the next check change nothing; a bound on the sub-iterations is honoured exactly (the loop is cut there).
#include "common.h"

#include <vector>

namespace riggs {

#define THIN_THREADS 1024
#define THIN_MAX_PER_LANE 40                  // 160 KiB / 4 B / 1024 lanes
#define THIN_LDS_BUDGET (160 * 1024)
#define THIN_LDS_TAIL 16                      // the two "pair deleted something" flags behind the plane
#define THIN_MAX_SIDE 32768
#define THIN_STEP_THREADS 256

static inline int thin_words_per_row(int W) { return (W + 31) / 32; }
// words of a padded plane, rounded up to 4 (16 bytes)
static inline size_t thin_plane_words(int H, int W) {
  const size_t S = (size_t)thin_words_per_row(W) + 1;
  return (((size_t)H + 2) * S + 1 + 3) / 4 * 4;
}
static inline size_t thin_lds_bytes(int H, int W) { return thin_plane_words(H, W) * 4 + THIN_LDS_TAIL; }

// The new value of the word `c` (non-zero) at index `at` of a padded plane; sub = 0 / 1: G3 / G3'.
__device__ __forceinline__ uint32_t thin_word(uint32_t c, const uint32_t* plane, int at, int S, int sub) {
  const uint32_t ul = plane[at - S - 1], u = plane[at - S], ur = plane[at - S + 1], l = plane[at - 1], r = plane[at + 1];
  const uint32_t dl = plane[at + S - 1], d = plane[at + S], dr = plane[at + S + 1];
  // bit k of x_i = the neighbour of column 32 j + k: column + 1 is the next bit up (the word shifted right), bit 31 from the next word
  const uint32_t x0 = (c >> 1) | (r << 31), x4 = (c << 1) | (l >> 31);
  const uint32_t x2 = u, x1 = (u >> 1) | (ur << 31), x3 = (u << 1) | (ul >> 31);
  const uint32_t x6 = d, x7 = (d >> 1) | (dr << 31), x5 = (d << 1) | (dl >> 31);
  // G1: exactly one of b0 .. b3
  const uint32_t b0 = ~x0 & (x1 | x2), b1 = ~x2 & (x3 | x4), b2 = ~x4 & (x5 | x6), b3 = ~x6 & (x7 | x0);
  const uint32_t b01 = b0 | b1, b012 = b01 | b2;
  const uint32_t g1 = (b012 | b3) & ~((b0 & b1) | (b01 & b2) | (b012 & b3));
  // G2: min(n1, n2) in {2, 3}  <=>  n1 >= 2 and n2 >= 2 and not (n1 == 4 and n2 == 4)
  const uint32_t p0 = x1 | x0, p1 = x3 | x2, p2 = x5 | x4, p3 = x7 | x6;  // n1's terms
  const uint32_t q0 = x1 | x2, q1 = x3 | x4, q2 = x5 | x6, q3 = x7 | x0;  // n2's terms
  const uint32_t p01 = p0 | p1, q01 = q0 | q1;
  const uint32_t n1_ge2 = (p0 & p1) | (p01 & p2) | ((p01 | p2) & p3), n2_ge2 = (q0 & q1) | (q01 & q2) | ((q01 | q2) & q3);
  const uint32_t g2 = n1_ge2 & n2_ge2 & ~(p0 & p1 & p2 & p3 & q0 & q1 & q2 & q3);
  // G3 on the neighbourhood turned by 180 degrees in the second sub-iteration
  const uint32_t a0 = sub ? x4 : x0, a1 = sub ? x5 : x1, a2 = sub ? x6 : x2, a7 = sub ? x3 : x7;
  const uint32_t g3 = ~((a1 | a2 | ~a7) & a0);
  return c & ~(g1 & g2 & g3);
}

// Word j of a row of W bytes (set: non-zero).  aligned4: the row starts 4-byte aligned and W % 4 == 0 (whole-dword reads).
__device__ __forceinline__ uint32_t thin_pack_word(const uint8_t* __restrict__ row, int j, int W, bool aligned4) {
  const int c0 = 32 * j, n = min(32, W - c0);
  uint32_t w = 0u;
  if (aligned4) {
    const uint32_t* __restrict__ q = (const uint32_t*)(row + c0);
    for (int k = 0; 4 * k < n; k++) {
      const uint32_t v = q[k];
      const uint32_t m = ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u) >> 7;  // 1 in every non-zero byte
      w |= ((m * 0x01020408u) >> 24 & 0xFu) << (4 * k);                                   // its four bits side by side
    }
  } else {
    for (int k = 0; k < n; k++) w |= (uint32_t)(row[c0 + k] != 0) << k;
  }
  return w;
}
// ... and back: bytes of 0 / 1.
__device__ __forceinline__ void thin_unpack_word(uint32_t w, uint8_t* __restrict__ row, int j, int W, bool aligned4) {
  const int c0 = 32 * j, n = min(32, W - c0);
  if (aligned4) {
    uint32_t* __restrict__ q = (uint32_t*)(row + c0);
    for (int k = 0; 4 * k < n; k++) q[k] = (((w >> (4 * k)) & 0xFu) * 0x00204081u) & 0x01010101u;
  } else {
    for (int k = 0; k < n; k++) row[c0 + k] = (uint8_t)((w >> k) & 1u);
  }
}

// Both paths sweep the padded plane LINEARLY from the first interior word: index i in [0, H S) is the word at 1 + S + i, word
// j = i % S of row i / S, where j = Wd is the row's pad word (0, never set: thin_word is not evaluated on a zero word).  The sweep
// itself therefore needs no division; only packing and unpacking split i into (row, word).
__global__ __launch_bounds__(THIN_THREADS) void thin_lds_kernel(int H, int W, int Wd, int plane_words,
                                                                const uint8_t* __restrict__ mask, uint8_t* __restrict__ out,
                                                                int first, int max_subiters, int aligned4) {
  extern __shared__ __attribute__((aligned(16))) uint32_t thin_lds[];
  const int tid = threadIdx.x, S = Wd + 1, n = H * S, nk = (n + THIN_THREADS - 1) / THIN_THREADS;
  const int mine = S + 1 + tid;   // this lane's k-th word: thin_lds[mine + k * THIN_THREADS]
  const size_t image = (size_t)blockIdx.x * (size_t)H * (size_t)W;
  mask += image;
  out += image;
  for (int i = tid; i < plane_words + 2; i += THIN_THREADS) thin_lds[i] = 0u;
  __syncthreads();
#pragma unroll 1
  for (int i = tid; i < n; i += THIN_THREADS) {
    const int r = i / S, j = i - r * S;
    if (j < Wd) thin_lds[S + 1 + i] = thin_pack_word(mask + (size_t)r * W, j, W, aligned4 != 0);
  }
  __syncthreads();
  uint32_t cur[THIN_MAX_PER_LANE];
#pragma unroll
  for (int k = 0; k < THIN_MAX_PER_LANE; k++) cur[k] = (k < nk && k * THIN_THREADS + tid < n) ? thin_lds[mine + k * THIN_THREADS] : 0u;
  uint32_t pair_changed = 0u;
  for (int s = 0; max_subiters < 0 || s < max_subiters; s++) {
    const int sub = (first + s) & 1;
    unsigned long long changed = 0ull;
#pragma unroll
    for (int k = 0; k < THIN_MAX_PER_LANE; k++) {
      if (k < nk && cur[k] != 0u) {   // (the words a lane has past n, and the pad words, are 0)
        const uint32_t w = thin_word(cur[k], thin_lds, mine + k * THIN_THREADS, S, sub);
        if (w != cur[k]) changed |= 1ull << k;
        cur[k] = w;
      }
    }
    __syncthreads();   // every lane has read the old state
    if (changed) {
      pair_changed = 1u;
#pragma unroll
      for (int k = 0; k < THIN_MAX_PER_LANE; k++)
        if (changed >> k & 1ull) thin_lds[mine + k * THIN_THREADS] = cur[k];
    }
    if (s & 1) {
      // the pair's verdict in flag word (pair & 1) behind the plane; the other flag is cleared for the next pair (every reader
      // of it has since passed the barrier above)
      const int f = (s >> 1) & 1;
      if (pair_changed) thin_lds[plane_words + f] = 1u;
      if (tid == 0) thin_lds[plane_words + (f ^ 1)] = 0u;
      pair_changed = 0u;
      __syncthreads();
      if (thin_lds[plane_words + f] == 0u) break;
    } else {
      __syncthreads();
    }
  }
  // (the plane in LDS is the final state: every changed word was written back, and the loop ends behind a barrier)
#pragma unroll 1
  for (int i = tid; i < n; i += THIN_THREADS) {
    const int r = i / S, j = i - r * S;
    if (j < Wd) thin_unpack_word(thin_lds[S + 1 + i], out + (size_t)r * W, j, W, aligned4 != 0);
  }
}

// ---- the global-memory path: padded planes in the workspace, one word per lane, grid (blocks, batch) ----
__global__ __launch_bounds__(THIN_STEP_THREADS) void thin_pack_kernel(int H, int W, int Wd, size_t plane_words,
                                                                      const uint8_t* __restrict__ mask, uint32_t* __restrict__ planes,
                                                                      int aligned4) {
  const int i = blockIdx.x * THIN_STEP_THREADS + threadIdx.x, S = Wd + 1;
  if (i >= H * S) return;
  const int r = i / S, j = i - r * S;
  if (j >= Wd) return;
  const uint8_t* row = mask + ((size_t)blockIdx.y * H + r) * (size_t)W;
  planes[(size_t)blockIdx.y * plane_words + (size_t)(S + 1 + i)] = thin_pack_word(row, j, W, aligned4 != 0);
}

__global__ __launch_bounds__(THIN_STEP_THREADS) void thin_unpack_kernel(int H, int W, int Wd, size_t plane_words,
                                                                        const uint32_t* __restrict__ planes, uint8_t* __restrict__ out,
                                                                        int aligned4) {
  const int i = blockIdx.x * THIN_STEP_THREADS + threadIdx.x, S = Wd + 1;
  if (i >= H * S) return;
  const int r = i / S, j = i - r * S;
  if (j >= Wd) return;
  uint8_t* row = out + ((size_t)blockIdx.y * H + r) * (size_t)W;
  thin_unpack_word(planes[(size_t)blockIdx.y * plane_words + (size_t)(S + 1 + i)], row, j, W, aligned4 != 0);
}

// src -> dst, both padded (a pad word of the sweep is rewritten with its 0, the others are 0 from the start and never written);
// deleted[image] |= 1 if counting.
__global__ __launch_bounds__(THIN_STEP_THREADS) void thin_step_kernel(int H, int Wd, size_t plane_words,
                                                                      const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                                      int sub, int32_t* __restrict__ deleted) {
  const int i = blockIdx.x * THIN_STEP_THREADS + threadIdx.x, S = Wd + 1;
  bool changed = false;
  if (i < H * S) {
    const size_t at = (size_t)blockIdx.y * plane_words + (size_t)(S + 1 + i);
    const uint32_t c = src[at];
    const uint32_t w = c ? thin_word(c, src + (size_t)blockIdx.y * plane_words, S + 1 + i, S, sub) : 0u;
    dst[at] = w;
    changed = w != c;
  }
  if (deleted && __ballot(changed) != 0ull && (threadIdx.x & (RIGGS_WAVE - 1)) == 0) atomicOr(deleted + blockIdx.y, 1);
}

// ---- compaction: the set pixels of (B, H, W) bytes as float32 (row, col) / resolution rows, row-major ascending ----
// One workgroup per image walks the words in order, 1024 at a time: popcount per word, a block scan, then every lane writes
// its word's pixels from the lowest bit up.  Rows at and beyond min(count, capacity) are not written.
__global__ __launch_bounds__(THIN_THREADS) void thin_elements_kernel(int H, int W, int Wd, const uint8_t* __restrict__ img,
                                                                     double resolution, int capacity, float* __restrict__ points,
                                                                     int32_t* __restrict__ counts, int aligned4) {
  __shared__ int wave_total[THIN_THREADS / RIGGS_WAVE];
  const int tid = threadIdx.x, lane = tid & (RIGGS_WAVE - 1), wave = tid / RIGGS_WAVE, n = H * Wd;
  img += (size_t)blockIdx.x * (size_t)H * (size_t)W;
  points += (size_t)blockIdx.x * (size_t)capacity * 2;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += THIN_THREADS) {
    const int i = i0 + tid;
    int r = 0, j = 0;
    uint32_t w = 0u;
    if (i < n) {
      r = i / Wd;
      j = i - r * Wd;
      w = thin_pack_word(img + (size_t)r * W, j, W, aligned4 != 0);
    }
    const int mine = __popc(w);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < RIGGS_WAVE; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    __syncthreads();   // (the previous round's readers of wave_total are done)
    if (lane == RIGGS_WAVE - 1) wave_total[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < THIN_THREADS / RIGGS_WAVE; v++) {
      const int t = wave_total[v];
      if (v < wave) before += t;
      total += t;
    }
    int at = base + before + incl - mine;
    while (w) {
      const int k = __ffs(w) - 1;
      w &= w - 1u;
      if (at < capacity) {
        points[2 * (size_t)at] = (float)((double)r / resolution);
        points[2 * (size_t)at + 1] = (float)((double)(32 * j + k) / resolution);
      }
      at++;
    }
    base += total;
  }
  if (tid == 0) counts[blockIdx.x] = min(base, capacity);
}

static bool thin_aligned4(const void* p, int W) { return W % 4 == 0 && ((uintptr_t)p & 3u) == 0; }

}  // namespace riggs

using namespace riggs;

extern "C" {

int32_t riggs_thin_path(int32_t H, int32_t W) {
  if (H < 1 || W < 1 || H > THIN_MAX_SIDE || W > THIN_MAX_SIDE) return -1;
  return thin_lds_bytes(H, W) <= THIN_LDS_BUDGET ? RIGGS_THIN_PATH_LDS : RIGGS_THIN_PATH_GLOBAL;
}

size_t riggs_thin_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t path) {
  if (B < 1 || riggs_thin_path(H, W) < 0) return 0;
  if (path == RIGGS_THIN_PATH_AUTO) path = riggs_thin_path(H, W);
  if (path != RIGGS_THIN_PATH_GLOBAL) return 0;
  return 2 * (size_t)B * thin_plane_words(H, W) * sizeof(uint32_t) + align_up((size_t)B * sizeof(int32_t));
}

int riggs_thin(int32_t B, int32_t H, int32_t W, const uint8_t* mask_u8, uint8_t* out_u8, int32_t first_subiter,
               int32_t max_subiters, int32_t path, int32_t check_every, void* workspace, riggs_stream stream) {
  RIGGS_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= THIN_MAX_SIDE && W <= THIN_MAX_SIDE,
                "riggs_thin: needs 1 <= B <= 65535 and 1 <= H, W <= 32768");
  RIGGS_REQUIRE(mask_u8 && out_u8, "riggs_thin: NULL argument");
  RIGGS_REQUIRE(first_subiter == 0 || first_subiter == 1, "riggs_thin: first_subiter is 0 or 1");
  RIGGS_REQUIRE(path == RIGGS_THIN_PATH_AUTO || path == RIGGS_THIN_PATH_LDS || path == RIGGS_THIN_PATH_GLOBAL, "riggs_thin: unknown path");
  const int fits = riggs_thin_path(H, W) == RIGGS_THIN_PATH_LDS;
  if (path == RIGGS_THIN_PATH_AUTO) path = fits ? RIGGS_THIN_PATH_LDS : RIGGS_THIN_PATH_GLOBAL;
  RIGGS_REQUIRE(path == RIGGS_THIN_PATH_GLOBAL || fits, "riggs_thin: the image's bit plane does not fit the LDS path (riggs_thin_path)");
  hipStream_t s = (hipStream_t)stream;
  const int Wd = thin_words_per_row(W), n = H * (Wd + 1);   // the words of a sweep
  const int a4 = thin_aligned4(mask_u8, W) && thin_aligned4(out_u8, W);
  if (max_subiters < 0) max_subiters = -1;
  if (path == RIGGS_THIN_PATH_LDS) {
    static unsigned long long attr_set = 0ull;
    if (once_per_device(attr_set))
      RIGGS_HIP_CHECK(hipFuncSetAttribute((const void*)thin_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, THIN_LDS_BUDGET));
    hipLaunchKernelGGL(thin_lds_kernel, dim3(B), dim3(THIN_THREADS), thin_lds_bytes(H, W), s, (int)H, (int)W, Wd,
                       (int)thin_plane_words(H, W), mask_u8, out_u8, (int)first_subiter, (int)max_subiters, a4);
    RIGGS_HIP_CHECK(hipGetLastError());
    return 0;
  }
  RIGGS_REQUIRE(workspace, "riggs_thin: the global path needs riggs_thin_workspace_bytes(B, H, W, path) bytes of workspace");
  RIGGS_REQUIRE(check_every >= 1, "riggs_thin: check_every >= 1");
  const size_t P = thin_plane_words(H, W);
  uint32_t* plane[2] = {(uint32_t*)workspace, (uint32_t*)workspace + (size_t)B * P};
  int32_t* deleted = (int32_t*)((uint32_t*)workspace + 2 * (size_t)B * P);
  RIGGS_HIP_CHECK(hipMemsetAsync(workspace, 0, riggs_thin_workspace_bytes(B, H, W, RIGGS_THIN_PATH_GLOBAL), s));
  const dim3 grid((n + THIN_STEP_THREADS - 1) / THIN_STEP_THREADS, B), block(THIN_STEP_THREADS);
  hipLaunchKernelGGL(thin_pack_kernel, grid, block, 0, s, (int)H, (int)W, Wd, P, mask_u8, plane[0], a4);
  std::vector<int32_t> host((size_t)B);
  int done = 0, src = 0;
  while (max_subiters < 0 || done < max_subiters) {
    long long chunk = 2ll * check_every;
    if (max_subiters >= 0 && chunk > max_subiters - done) chunk = max_subiters - done;
    for (int k = 0; k < (int)chunk; k++, done++, src ^= 1) {
      const bool counting = (chunk & 1) == 0 && k >= (int)chunk - 2;   // the last whole pair of the chunk
      hipLaunchKernelGGL(thin_step_kernel, grid, block, 0, s, (int)H, Wd, P, (const uint32_t*)plane[src], plane[src ^ 1],
                         (first_subiter + done) & 1, counting ? deleted : (int32_t*)nullptr);
    }
    RIGGS_HIP_CHECK(hipGetLastError());
    if (max_subiters >= 0 && done >= max_subiters) break;
    RIGGS_HIP_CHECK(hipMemcpyAsync(host.data(), deleted, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RIGGS_HIP_CHECK(hipStreamSynchronize(s));
    bool any = false;
    for (int b = 0; b < B; b++) any = any || host[b] != 0;
    if (!any) break;
    RIGGS_HIP_CHECK(hipMemsetAsync(deleted, 0, (size_t)B * sizeof(int32_t), s));
  }
  hipLaunchKernelGGL(thin_unpack_kernel, grid, block, 0, s, (int)H, (int)W, Wd, P, (const uint32_t*)plane[src], out_u8, a4);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_thin_elements(int32_t B, int32_t H, int32_t W, const uint8_t* img_u8, double resolution, int32_t capacity, float* points,
                        int32_t* counts, riggs_stream stream) {
  RIGGS_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= THIN_MAX_SIDE && W <= THIN_MAX_SIDE, "riggs_thin_elements: needs B >= 1 and 1 <= H, W <= 32768");
  RIGGS_REQUIRE(capacity >= 0 && resolution > 0.0, "riggs_thin_elements: needs capacity >= 0 and resolution > 0");
  RIGGS_REQUIRE(img_u8 && counts && (points || capacity == 0), "riggs_thin_elements: NULL argument");
  hipLaunchKernelGGL(thin_elements_kernel, dim3(B), dim3(THIN_THREADS), 0, (hipStream_t)stream, (int)H, (int)W, thin_words_per_row(W),
                     img_u8, resolution, (int)capacity, points, counts, (int)thin_aligned4(img_u8, W));
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
