// The stage-1 node network (DeformNetwork): positional embedding, time net, an 8-layer ReLU trunk with one skip and the
// output heads, forward and backward, in fp32 on the matrix pipe (v_mfma_f32_16x16x4_f32: an exact k-ordered fmaf chain).
//
// Three launches per call:
//   forward         one workgroup per tile of 16 or 32 rows; the tile's activations stay in LDS between layers, the weights are
//                   read in place from the fp32 masters (row-major (out, in)), shared through L2 by every workgroup.
//   backward, data  the same tiling, from the heads' cotangents back to every layer's pre-activation gradient.
//   backward, params one workgroup per (layer, 32 outputs x 32 inputs): its four waves walk the four quarters of the rows in
//                   ascending order and the quarters are added in wave order: deterministic, no float atomics.  The bias
//                   gradient is the same chain against a column of ones.
// The inputs x, t are never differentiated.
//
// MFMA operand maps (16x16x4, lane l: j = l & 15, q = l >> 4): A[i = j][k = q], B[k = q][col = j], D[row = 4 q + reg][col = j].
// A 16-wide chunk of the summed index is fed as four instructions whose lane group q supplies k = 16 c' + 4 q + c (c = the
// instruction), so that both operands are one 16-byte read per lane and chunk.  The order of the chain is fixed, not ascending.
#include "common.h"

namespace riggs {

constexpr int NM_D = 8;          // trunk layers
constexpr int NM_SKIP = 4;       // the input is concatenated in front of the output of this layer
constexpr int NM_XCH = 63;       // PE_10 of 3 coordinates
constexpr int NM_EMB = 96;       // stored embedded input, padded (93 with the time net, 84 without)
constexpr int NM_EMB_LD = 100;   // its LDS row stride
constexpr int NM_HS = 260;       // LDS row stride of an activation tile (256 + 4)
constexpr int NM_TNH = 256;      // hidden width of the time net
constexpr int NM_TEMB = 16;      // stored PE_6(t), padded (13)
constexpr int NM_TOUT = 30;      // output width of the time net
constexpr int NM_HEADS = 5;      // warp 3, scaling 3, rotation 4, local_rotation 4, opacity 1: columns 0..14 of one 16-wide product
constexpr int NM_RMAX = 65536;

typedef float nm_f4 __attribute__((ext_vector_type(4)));

struct NmNet {
  int in_ch, is_blender, use_tanh;
  float scale_log;
  const float *tn_w0, *tn_b0, *tn_w1, *tn_b1;
  const float* w[NM_D];
  const float* b[NM_D];
  const float* hw[NM_HEADS];
  const float* hb[NM_HEADS];
};
struct NmOut { float* p[NM_HEADS]; };
struct NmCot { const float* p[NM_HEADS]; };

struct NmActs { size_t emb, temb, tnh, spre, a, total; };
__host__ __device__ static inline NmActs nm_acts(size_t R, int W) {
  NmActs L;
  size_t o = 0;
  L.emb = o; o += R * NM_EMB;
  L.temb = o; o += R * NM_TEMB;
  L.tnh = o; o += R * NM_TNH;
  L.spre = o; o += R * 4;
  L.a = o; o += (size_t)NM_D * R * W;
  L.total = o;
  return L;
}
struct NmWs { size_t dpre, dtn0, dtn1, dhead, total; };
__host__ __device__ static inline NmWs nm_ws(size_t R, int W) {
  NmWs L;
  size_t o = 0;
  L.dpre = o; o += (size_t)NM_D * R * W;
  L.dtn0 = o; o += R * NM_TNH;
  L.dtn1 = o; o += R * 32;
  L.dhead = o; o += R * 16;
  L.total = o;
  return L;
}

#define NM_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// head column c (0..15) -> head index, row inside the head, width of the head
__device__ __forceinline__ int nm_head_of(int c) { return c < 3 ? 0 : c < 6 ? 1 : c < 10 ? 2 : c < 14 ? 3 : 4; }
__device__ __forceinline__ int nm_head_first(int h) { return h == 0 ? 0 : h == 1 ? 3 : h == 2 ? 6 : h == 3 ? 10 : 14; }
__device__ __forceinline__ int nm_head_width(int h) { return h == 0 ? 3 : h == 1 ? 3 : h == 2 ? 4 : h == 3 ? 4 : 1; }
template <typename T>
__device__ __forceinline__ T nm_pick(T const (&p)[NM_HEADS], int h) {
  return h == 0 ? p[0] : h == 1 ? p[1] : h == 2 ? p[2] : h == 3 ? p[3] : p[4];
}

// acc[m][n] += As (LDS: rows 16 m + j, stride lda) x rows of a row-major (out, in) weight: wrow[n] is this lane's weight row
// (output 16 n + j of the wave's columns) at input 0, or NULL.  K inputs are real, Kpad (a multiple of 16) are walked; As holds
// zeros beyond K.  VEC: 16-byte weight reads (row stride and K multiples of 4, no padding).
template <int MT, int NT, bool VEC>
__device__ __forceinline__ void nm_prod(nm_f4 (&acc)[MT][NT], const float* As, int lda, const float* const (&wrow)[NT], int K,
                                        int Kpad, int lane) {
  const int j = lane & 15, q = lane >> 4;
  for (int kb = 0; kb < Kpad; kb += 16) {
    const int k = kb + 4 * q;
    nm_f4 a[MT], b[NT];
#pragma unroll
    for (int m = 0; m < MT; m++) a[m] = *reinterpret_cast<const nm_f4*>(As + (m * 16 + j) * lda + k);
#pragma unroll
    for (int n = 0; n < NT; n++) {
      if (VEC) {
        b[n] = *reinterpret_cast<const nm_f4*>(wrow[n] + k);
      } else {
#pragma unroll
        for (int c = 0; c < 4; c++) b[n][c] = (wrow[n] && k + c < K) ? wrow[n][k + c] : 0.f;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
      for (int n = 0; n < NT; n++)
#pragma unroll
        for (int m = 0; m < MT; m++) acc[m][n] = NM_MFMA(a[m][c], b[n][c], acc[m][n]);
  }
}

// acc[m][n] += As (LDS) x M, M row-major [K][.] with row stride ld: colp[n] is this lane's column of M at row 0, or NULL.
template <int MT, int NT>
__device__ __forceinline__ void nm_prod_t(nm_f4 (&acc)[MT][NT], const float* As, int lda, const float* const (&colp)[NT], int ld,
                                          int K, int lane) {
  const int j = lane & 15, q = lane >> 4;
  for (int kb = 0; kb < K; kb += 16) {
    const int k = kb + 4 * q;
    nm_f4 a[MT], b[NT];
#pragma unroll
    for (int m = 0; m < MT; m++) a[m] = *reinterpret_cast<const nm_f4*>(As + (m * 16 + j) * lda + k);
#pragma unroll
    for (int n = 0; n < NT; n++)
#pragma unroll
      for (int c = 0; c < 4; c++) b[n][c] = colp[n] ? colp[n][(size_t)(k + c) * ld] : 0.f;
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
      for (int n = 0; n < NT; n++)
#pragma unroll
        for (int m = 0; m < MT; m++) acc[m][n] = NM_MFMA(a[m][c], b[n][c], acc[m][n]);
  }
}

template <int MT, int NT>
__device__ __forceinline__ void nm_zero(nm_f4 (&acc)[MT][NT]) {
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int n = 0; n < NT; n++) acc[m][n] = nm_f4{0.f, 0.f, 0.f, 0.f};
}

// ---------------------------------------------------------------------------------------------------------- forward
template <int W, int MT>
__global__ __launch_bounds__(256) void nm_forward_kernel(NmNet p, int R, const float* __restrict__ x, const float* __restrict__ t,
                                                         int t_stride, float* __restrict__ acts, NmOut out) {
  constexpr int TR = 16 * MT, NT = W / 64;
  extern __shared__ float nm_smem[];
  float* emb = nm_smem;                 // [TR][NM_EMB_LD]
  float* hA = emb + TR * NM_EMB_LD;     // [TR][NM_HS]
  float* hB = hA + TR * NM_HS;          // [TR][NM_HS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * TR;
  const NmActs AL = nm_acts((size_t)R, W);
  const int in_ch = p.in_ch;

  for (int i = tid; i < TR * NM_EMB_LD; i += 256) emb[i] = 0.f;
  __syncthreads();
  // PE_10(x): [x, sin(2^k x), cos(2^k x)] k = 0..9
  for (int i = tid; i < TR * NM_XCH; i += 256) {
    const int row = i / NM_XCH, c = i - row * NM_XCH, r = r0 + row;
    if (r < R) {
      float v;
      if (c < 3) {
        v = x[(size_t)r * 3 + c];
      } else {
        const int cc = c - 3, kf = cc / 6, s = cc - kf * 6, d = s >= 3 ? s - 3 : s;
        const float arg = x[(size_t)r * 3 + d] * (float)(1 << kf);
        v = s >= 3 ? cosf(arg) : sinf(arg);
      }
      emb[row * NM_EMB_LD + c] = v;
    }
  }
  // PE(t): 13 columns into the time net (is_blender), else 21 columns straight into the input
  const int tc = p.is_blender ? 13 : 21;
  float* temb_s = hB;                   // [TR][NM_TEMB] (is_blender)
  for (int i = tid; i < TR * tc; i += 256) {
    const int row = i / tc, c = i - row * tc, r = r0 + row;
    float v = 0.f;
    if (r < R) {
      const float tv = t[(size_t)r * t_stride];
      if (c == 0) {
        v = tv;
      } else {
        const int cc = c - 1, kf = cc >> 1;
        const float arg = tv * (float)(1 << kf);
        v = (cc & 1) ? cosf(arg) : sinf(arg);
      }
    }
    if (p.is_blender) {
      temb_s[row * NM_TEMB + c] = v;
      if (r < R) acts[AL.temb + (size_t)r * NM_TEMB + c] = v;
    } else {
      emb[row * NM_EMB_LD + NM_XCH + c] = v;
    }
  }
  __syncthreads();
  if (p.is_blender) {
    {  // timenet.0: 13 -> 256, ReLU (vector ALU; thread = hidden unit)
      float w0[13];
#pragma unroll
      for (int c = 0; c < 13; c++) w0[c] = p.tn_w0[tid * 13 + c];
      const float b0 = p.tn_b0[tid];
      for (int row = 0; row < TR; row++) {
        float s = b0;
#pragma unroll
        for (int c = 0; c < 13; c++) s = fmaf(temb_s[row * NM_TEMB + c], w0[c], s);
        s = fmaxf(s, 0.f);
        hA[row * NM_HS + tid] = s;
        if (r0 + row < R) acts[AL.tnh + (size_t)(r0 + row) * NM_TNH + tid] = s;
      }
    }
    __syncthreads();
    if (wave < 2) {  // timenet.2: 256 -> 30, two 16-column tiles
      nm_f4 acc[MT][1];
      nm_zero(acc);
      const int col = wave * 16 + j;
      const float* wrow[1] = {col < NM_TOUT ? p.tn_w1 + (size_t)col * NM_TNH : nullptr};
      nm_prod<MT, 1, false>(acc, hA, NM_HS, wrow, NM_TNH, NM_TNH, lane);
      if (col < NM_TOUT) {
        const float bb = p.tn_b1[col];
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
          for (int g = 0; g < 4; g++) {
            const int row = m * 16 + q * 4 + g;
            emb[row * NM_EMB_LD + NM_XCH + col] = (r0 + row < R) ? acc[m][0][g] + bb : 0.f;
          }
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < TR * NM_EMB; i += 256) {
    const int row = i / NM_EMB, c = i - row * NM_EMB;
    if (r0 + row < R) acts[AL.emb + (size_t)(r0 + row) * NM_EMB + c] = emb[row * NM_EMB_LD + c];
  }

  // trunk
  float* cur = hA;
  float* nxt = hB;
  const int n0 = wave * (W / 4);
#pragma unroll
  for (int l = 0; l < NM_D; l++) {
    nm_f4 acc[MT][NT];
    nm_zero(acc);
    if (l == 0 || l == NM_SKIP + 1) {
      const int ldw = l == 0 ? in_ch : in_ch + W;
      const float* wrow[NT];
#pragma unroll
      for (int n = 0; n < NT; n++) wrow[n] = p.w[l] + (size_t)(n0 + n * 16 + j) * ldw;
      nm_prod<MT, NT, false>(acc, emb, NM_EMB_LD, wrow, in_ch, NM_EMB, lane);
      if (l != 0) {
#pragma unroll
        for (int n = 0; n < NT; n++) wrow[n] += in_ch;
        nm_prod<MT, NT, false>(acc, cur, NM_HS, wrow, W, W, lane);
      }
    } else {
      const float* wrow[NT];
#pragma unroll
      for (int n = 0; n < NT; n++) wrow[n] = p.w[l] + (size_t)(n0 + n * 16 + j) * W;
      nm_prod<MT, NT, true>(acc, cur, NM_HS, wrow, W, W, lane);
    }
    float* ag = acts + AL.a + (size_t)l * R * W;
#pragma unroll
    for (int n = 0; n < NT; n++) {
      const int col = n0 + n * 16 + j;
      const float bb = p.b[l][col];
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int row = m * 16 + q * 4 + g;
          const float v = fmaxf(acc[m][n][g] + bb, 0.f);
          nxt[row * NM_HS + col] = v;
          if (r0 + row < R) ag[(size_t)(r0 + row) * W + col] = v;
        }
    }
    __syncthreads();
    float* tmp = cur; cur = nxt; nxt = tmp;
  }

  // heads: one 16-column product per 16 rows
  if (wave < MT) {
    nm_f4 acc[1][1];
    nm_zero(acc);
    const int h = nm_head_of(j), first = nm_head_first(h), wd = nm_head_width(h);
    const float* hw = nm_pick(p.hw, h);
    const float* hb = nm_pick(p.hb, h);
    const bool live = j < 15 && hw != nullptr;
    const float* wrow[1] = {live ? hw + (size_t)(j - first) * W : nullptr};
    nm_prod<1, 1, false>(acc, cur + wave * 16 * NM_HS, NM_HS, wrow, W, W, lane);
    float* op = nm_pick(out.p, h);
    if (live) {
      const float bb = hb[j - first];
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int r = r0 + wave * 16 + q * 4 + g;
        if (r < R) {
          float v = acc[0][0][g] + bb;
          if (h == 1 && p.use_tanh) {
            acts[AL.spre + (size_t)r * 4 + (j - first)] = v;
            v = tanhf(v) * p.scale_log;
          }
          op[(size_t)r * wd + (j - first)] = v;
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------------------------- backward, data
template <int W, int MT>
__global__ __launch_bounds__(256) void nm_backward_data_kernel(NmNet p, int R, const float* __restrict__ acts, NmCot cot,
                                                               float* __restrict__ ws) {
  constexpr int TR = 16 * MT, NT = W / 64;
  extern __shared__ float nm_smem[];
  float* dA = nm_smem;              // [TR][NM_HS]
  float* dB = dA + TR * NM_HS;      // [TR][NM_HS]
  float* gs = dB + TR * NM_HS;      // [TR][20]
  float* dte = gs + TR * 20;        // [TR][36]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * TR;
  const NmActs AL = nm_acts((size_t)R, W);
  const NmWs WL = nm_ws((size_t)R, W);
  const int in_ch = p.in_ch;

  // the heads' cotangents, one 16-column row per network row (absent heads and cotangents: zero)
  for (int i = tid; i < TR * 16; i += 256) {
    const int row = i >> 4, c = i & 15, r = r0 + row;
    const int h = nm_head_of(c), first = nm_head_first(h), wd = nm_head_width(h);
    const float* gp = nm_pick(cot.p, h);
    const float* hw = nm_pick(p.hw, h);
    float v = 0.f;
    if (r < R && c < 15 && gp != nullptr && hw != nullptr) {
      v = gp[(size_t)r * wd + (c - first)];
      if (h == 1 && p.use_tanh) {
        const float th = tanhf(acts[AL.spre + (size_t)r * 4 + (c - first)]);
        v = v * p.scale_log * (1.f - th * th);
      }
    }
    gs[row * 20 + c] = v;
    if (r < R) ws[WL.dhead + (size_t)r * 16 + c] = v;
  }
  __syncthreads();

  const int n0 = wave * (W / 4);
  float* cur = dA;
  float* nxt = dB;
  {  // dL/d(last activation) = g (TR x 16) x head weights (16 x W), masked
    nm_f4 acc[MT][NT];
    nm_zero(acc);
    nm_f4 a[MT], b[NT];
#pragma unroll
    for (int m = 0; m < MT; m++) a[m] = *reinterpret_cast<const nm_f4*>(gs + (m * 16 + j) * 20 + 4 * q);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int k = 4 * q + c, h = nm_head_of(k), first = nm_head_first(h);
      const float* hw = nm_pick(p.hw, h);
      const bool live = k < 15 && hw != nullptr;
#pragma unroll
      for (int n = 0; n < NT; n++) b[n][c] = live ? hw[(size_t)(k - first) * W + n0 + n * 16 + j] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
      for (int n = 0; n < NT; n++)
#pragma unroll
        for (int m = 0; m < MT; m++) acc[m][n] = NM_MFMA(a[m][c], b[n][c], acc[m][n]);
    const float* ag = acts + AL.a + (size_t)(NM_D - 1) * R * W;
    float* dg = ws + WL.dpre + (size_t)(NM_D - 1) * R * W;
#pragma unroll
    for (int n = 0; n < NT; n++)
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int row = m * 16 + q * 4 + g, col = n0 + n * 16 + j;
          float v = 0.f;
          if (r0 + row < R) {
            v = ag[(size_t)(r0 + row) * W + col] > 0.f ? acc[m][n][g] : 0.f;
            dg[(size_t)(r0 + row) * W + col] = v;
          }
          cur[row * NM_HS + col] = v;
        }
  }
  __syncthreads();

  // dL/d(time net output), accumulated over the two layers that read the embedded input (waves 0, 1: 16 columns each)
  nm_f4 acct[MT][1];
  nm_zero(acct);
  const int tcol = wave * 16 + j;
  const bool twave = p.is_blender && wave < 2;

#pragma unroll
  for (int l = NM_D - 1; l >= 1; l--) {
    // cur = dL/d(pre-activation of layer l)
    const int ld = l == NM_SKIP + 1 ? in_ch + W : W, coff = l == NM_SKIP + 1 ? in_ch : 0;
    if (l == NM_SKIP + 1 && twave) {
      const float* colp[1] = {tcol < NM_TOUT ? p.w[l] + NM_XCH + tcol : nullptr};
      nm_prod_t<MT, 1>(acct, cur, NM_HS, colp, ld, W, lane);
    }
    nm_f4 acc[MT][NT];
    nm_zero(acc);
    const float* colp[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) colp[n] = p.w[l] + coff + n0 + n * 16 + j;
    nm_prod_t<MT, NT>(acc, cur, NM_HS, colp, ld, W, lane);
    const float* ag = acts + AL.a + (size_t)(l - 1) * R * W;
    float* dg = ws + WL.dpre + (size_t)(l - 1) * R * W;
#pragma unroll
    for (int n = 0; n < NT; n++)
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int row = m * 16 + q * 4 + g, col = n0 + n * 16 + j;
          float v = 0.f;
          if (r0 + row < R) {
            v = ag[(size_t)(r0 + row) * W + col] > 0.f ? acc[m][n][g] : 0.f;
            dg[(size_t)(r0 + row) * W + col] = v;
          }
          nxt[row * NM_HS + col] = v;
        }
    __syncthreads();
    float* tmp = cur; cur = nxt; nxt = tmp;
  }

  if (p.is_blender) {
    if (twave) {
      const float* colp[1] = {tcol < NM_TOUT ? p.w[0] + NM_XCH + tcol : nullptr};
      nm_prod_t<MT, 1>(acct, cur, NM_HS, colp, in_ch, W, lane);
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int row = m * 16 + q * 4 + g;
          const float v = acct[m][0][g];   // columns 30, 31: zero (no weight column)
          dte[row * 36 + tcol] = v;
          if (r0 + row < R) ws[WL.dtn1 + (size_t)(r0 + row) * 32 + tcol] = v;
        }
    }
    __syncthreads();
    // through timenet.2 (30 x 256) and the ReLU of timenet.0: thread = hidden unit
    float w1[NM_TOUT];
#pragma unroll
    for (int o = 0; o < NM_TOUT; o++) w1[o] = p.tn_w1[o * NM_TNH + tid];
    for (int row = 0; row < TR; row++) {
      const int r = r0 + row;
      if (r >= R) break;
      float s = 0.f;
#pragma unroll
      for (int o = 0; o < NM_TOUT; o++) s = fmaf(dte[row * 36 + o], w1[o], s);
      const float hv = acts[AL.tnh + (size_t)r * NM_TNH + tid];
      ws[WL.dtn0 + (size_t)r * NM_TNH + tid] = hv > 0.f ? s : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------- backward, parameters
// dW[o][i] = sum_r dpre[r][o] * inp[r][i], db[o] = sum_r dpre[r][o].
struct NmJob {
  const float* dpre;
  const float* inp;
  float* dW;
  float* db;
  int ldo, n_out, ldi, n_in, ldw;
};
constexpr int NM_JOBS = 16;
struct NmJobs {
  NmJob job[NM_JOBS];
  int start[NM_JOBS];   // first workgroup of the job (INT_MAX: unused)
};

__global__ __launch_bounds__(256) void nm_backward_param_kernel(NmJobs T, int R) {
  // One workgroup per (job, 32 outputs x 32 inputs).  Its four waves walk the four quarters of the rows, each in ascending
  // order, sixteen rows per step (the loads of a step are issued together); the quarters are added in wave order through LDS.
  __shared__ float part[3][24][64];
  const int bid = blockIdx.x;
  NmJob jb = T.job[0];
  int first = 0;
#pragma unroll
  for (int i = 1; i < NM_JOBS; i++)
    if (bid >= T.start[i]) { jb = T.job[i]; first = T.start[i]; }
  const int tiles_in = (jb.n_in + 31) >> 5;
  const int tile = bid - first, to = tile / tiles_in, ti = tile - to * tiles_in;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const int o0 = to * 32, i0 = ti * 32;
  const bool bias = jb.db != nullptr && ti == 0;
  const int oc0 = o0 + j, oc1 = o0 + 16 + j, ic0 = i0 + j, ic1 = i0 + 16 + j;
  const bool ov0 = oc0 < jb.n_out, ov1 = oc1 < jb.n_out, iv0 = ic0 < jb.n_in, iv1 = ic1 < jb.n_in;
  const nm_f4 z = {0.f, 0.f, 0.f, 0.f};
  nm_f4 acc[6] = {z, z, z, z, z, z};   // (o0, i0), (o0, i1), (o1, i0), (o1, i1), bias o0, bias o1
  const int rq = ((R + 15) / 16) * 4;   // rows per wave, a multiple of 4
  const int rb = wave * rq, re = min(R, rb + rq);
  for (int r = rb; r < re; r += 16) {
    float A0[4], A1[4], B0[4], B1[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int row = r + 4 * u + q;
      const bool ok = row < re;
      const float* dp = jb.dpre + (size_t)row * jb.ldo;
      const float* ip = jb.inp + (size_t)row * jb.ldi;
      A0[u] = (ok && ov0) ? dp[oc0] : 0.f;
      A1[u] = (ok && ov1) ? dp[oc1] : 0.f;
      B0[u] = (ok && iv0) ? ip[ic0] : 0.f;
      B1[u] = (ok && iv1) ? ip[ic1] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      acc[0] = NM_MFMA(A0[u], B0[u], acc[0]);
      acc[1] = NM_MFMA(A0[u], B1[u], acc[1]);
      acc[2] = NM_MFMA(A1[u], B0[u], acc[2]);
      acc[3] = NM_MFMA(A1[u], B1[u], acc[3]);
      if (bias) {
        acc[4] = NM_MFMA(A0[u], 1.0f, acc[4]);
        acc[5] = NM_MFMA(A1[u], 1.0f, acc[5]);
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int g = 0; g < 4; g++) part[wave - 1][a * 4 + g][lane] = acc[a][g];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int w = 0; w < 3; w++)
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int g = 0; g < 4; g++) acc[a][g] += part[w][a * 4 + g][lane];
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int oa = o0 + q * 4 + g, ob = oa + 16;
    if (oa < jb.n_out) {
      if (iv0) jb.dW[(size_t)oa * jb.ldw + ic0] = acc[0][g];
      if (iv1) jb.dW[(size_t)oa * jb.ldw + ic1] = acc[1][g];
      if (bias && j == 0) jb.db[oa] = acc[4][g];
    }
    if (ob < jb.n_out) {
      if (iv0) jb.dW[(size_t)ob * jb.ldw + ic0] = acc[2][g];
      if (iv1) jb.dW[(size_t)ob * jb.ldw + ic1] = acc[3][g];
      if (bias && j == 0) jb.db[ob] = acc[5][g];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- host
static inline int nm_mt(int R) { return R <= 4096 ? 1 : 2; }   // 16-row tiles while they leave CUs idle, else 32
static inline size_t nm_fwd_lds(int MT) { return (size_t)16 * MT * (NM_EMB_LD + 2 * NM_HS) * sizeof(float); }
static inline size_t nm_bwd_lds(int MT) { return (size_t)16 * MT * (2 * NM_HS + 20 + 36) * sizeof(float); }

static int nm_check(const riggs_node_mlp* net, int32_t R, const char* who) {
  RIGGS_REQUIRE(net != nullptr, "riggs_node_mlp: null network");
  RIGGS_REQUIRE(net->width == 64 || net->width == 128 || net->width == 256, "riggs_node_mlp: width must be 64, 128 or 256");
  RIGGS_REQUIRE(net->depth == NM_D, "riggs_node_mlp: depth must be 8");
  RIGGS_REQUIRE(R >= 1 && R <= NM_RMAX, "riggs_node_mlp: 1 <= rows <= 65536 per call");
  RIGGS_REQUIRE(net->is_blender == 0 || net->is_blender == 1, "riggs_node_mlp: is_blender is 0 or 1");
  (void)who;
  return 0;
}

static int nm_net(NmNet& p, const riggs_node_mlp* net) {
  p.is_blender = net->is_blender;
  p.in_ch = NM_XCH + (net->is_blender ? NM_TOUT : 21);
  p.use_tanh = net->max_d_scale > 0.f ? 1 : 0;
  p.scale_log = net->max_d_scale > 0.f ? (float)log((double)net->max_d_scale) : 0.f;
  p.tn_w0 = net->tn_w0; p.tn_b0 = net->tn_b0; p.tn_w1 = net->tn_w1; p.tn_b1 = net->tn_b1;
  if (net->is_blender) RIGGS_REQUIRE(p.tn_w0 && p.tn_b0 && p.tn_w1 && p.tn_b1, "riggs_node_mlp: is_blender needs the time net");
  for (int l = 0; l < NM_D; l++) {
    p.w[l] = net->w[l]; p.b[l] = net->b[l];
    RIGGS_REQUIRE(p.w[l] && p.b[l], "riggs_node_mlp: null trunk parameter");
  }
  for (int h = 0; h < NM_HEADS; h++) {
    p.hw[h] = net->head_w[h]; p.hb[h] = net->head_b[h];
    RIGGS_REQUIRE((p.hw[h] == nullptr) == (p.hb[h] == nullptr), "riggs_node_mlp: a head needs its weight and its bias");
    if (h < 3) RIGGS_REQUIRE(p.hw[h] != nullptr, "riggs_node_mlp: warp, scaling and rotation heads are required");
  }
  return 0;
}

template <int W, int MT>
static int nm_launch_forward(const NmNet& p, int R, const float* x, const float* t, int t_stride, float* acts, const NmOut& o,
                             hipStream_t s) {
  static unsigned long long done = 0;
  if (once_per_device(done))
    RIGGS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nm_forward_kernel<W, MT>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)nm_fwd_lds(MT)));
  hipLaunchKernelGGL((nm_forward_kernel<W, MT>), dim3((R + 16 * MT - 1) / (16 * MT)), dim3(256), nm_fwd_lds(MT), s, p, R, x, t,
                     t_stride, acts, o);
  return 0;
}
template <int W, int MT>
static int nm_launch_bwd_data(const NmNet& p, int R, const float* acts, const NmCot& c, float* ws, hipStream_t s) {
  static unsigned long long done = 0;
  if (once_per_device(done))
    RIGGS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nm_backward_data_kernel<W, MT>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)nm_bwd_lds(MT)));
  hipLaunchKernelGGL((nm_backward_data_kernel<W, MT>), dim3((R + 16 * MT - 1) / (16 * MT)), dim3(256), nm_bwd_lds(MT), s, p, R,
                     acts, c, ws);
  return 0;
}

}  // namespace riggs

using namespace riggs;

extern "C" {

size_t riggs_node_mlp_acts_floats(int32_t R, int32_t width, int32_t depth) {
  if (R < 1 || R > NM_RMAX || depth != NM_D || (width != 64 && width != 128 && width != 256)) return 0;
  return nm_acts((size_t)R, width).total;
}

size_t riggs_node_mlp_backward_workspace_floats(int32_t R, int32_t width, int32_t depth) {
  if (R < 1 || R > NM_RMAX || depth != NM_D || (width != 64 && width != 128 && width != 256)) return 0;
  return nm_ws((size_t)R, width).total;
}

size_t riggs_node_mlp_hidden_offset(int32_t R, int32_t width, int32_t depth) {
  if (R < 1 || R > NM_RMAX || depth != NM_D || (width != 64 && width != 128 && width != 256)) return 0;
  return nm_acts((size_t)R, width).a + (size_t)(NM_D - 1) * R * width;
}

int riggs_node_mlp_forward(const riggs_node_mlp* net, int32_t R, const float* x, const float* t, int32_t t_stride, float* acts,
                           float* d_xyz, float* d_scaling, float* d_rotation, float* local_rotation, float* d_opacity,
                           riggs_stream stream) {
  if (int rc = nm_check(net, R, "forward")) return rc;
  NmNet p;
  if (int rc = nm_net(p, net)) return rc;
  RIGGS_REQUIRE(x && t && acts, "riggs_node_mlp_forward: null pointer");
  RIGGS_REQUIRE(t_stride == 0 || t_stride == 1, "riggs_node_mlp_forward: t_stride is 0 (one shared time) or 1");
  NmOut o{{d_xyz, d_scaling, d_rotation, local_rotation, d_opacity}};
  for (int h = 0; h < NM_HEADS; h++)
    RIGGS_REQUIRE((o.p[h] != nullptr) == (p.hw[h] != nullptr), "riggs_node_mlp_forward: one output per head of the network");
  hipStream_t s = (hipStream_t)stream;
  const int MT = nm_mt(R);
  int rc = 0;
#define NM_CASE(WW)                                                                                   \
  case WW:                                                                                            \
    rc = MT == 1 ? nm_launch_forward<WW, 1>(p, R, x, t, t_stride, acts, o, s)                         \
                 : nm_launch_forward<WW, 2>(p, R, x, t, t_stride, acts, o, s);                        \
    break;
  switch (net->width) { NM_CASE(64) NM_CASE(128) NM_CASE(256) }
#undef NM_CASE
  if (rc) return rc;
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_node_mlp_backward(const riggs_node_mlp* net, int32_t R, const float* acts, const float* g_xyz, const float* g_scaling,
                            const float* g_rotation, const float* g_local_rotation, const float* g_opacity, float* workspace,
                            const riggs_node_mlp_grads* grads, riggs_stream stream) {
  if (int rc = nm_check(net, R, "backward")) return rc;
  NmNet p;
  if (int rc = nm_net(p, net)) return rc;
  RIGGS_REQUIRE(acts && workspace && grads, "riggs_node_mlp_backward: null pointer");
  const int W = net->width, in_ch = p.in_ch;
  for (int l = 0; l < NM_D; l++) RIGGS_REQUIRE(grads->w[l] && grads->b[l], "riggs_node_mlp_backward: null trunk gradient");
  for (int h = 0; h < NM_HEADS; h++)
    RIGGS_REQUIRE(!p.hw[h] || (grads->head_w[h] && grads->head_b[h]), "riggs_node_mlp_backward: null head gradient");
  if (p.is_blender)
    RIGGS_REQUIRE(grads->tn_w0 && grads->tn_b0 && grads->tn_w1 && grads->tn_b1, "riggs_node_mlp_backward: null time net gradient");
  hipStream_t s = (hipStream_t)stream;
  NmCot c{{g_xyz, g_scaling, g_rotation, g_local_rotation, g_opacity}};
  const int MT = nm_mt(R);
  int rc = 0;
#define NM_CASE(WW)                                                                   \
  case WW:                                                                            \
    rc = MT == 1 ? nm_launch_bwd_data<WW, 1>(p, R, acts, c, workspace, s)             \
                 : nm_launch_bwd_data<WW, 2>(p, R, acts, c, workspace, s);            \
    break;
  switch (W) { NM_CASE(64) NM_CASE(128) NM_CASE(256) }
#undef NM_CASE
  if (rc) return rc;

  const NmActs AL = nm_acts((size_t)R, W);
  const NmWs WL = nm_ws((size_t)R, W);
  NmJobs T;
  int nj = 0, nblocks = 0;
  auto add = [&](const float* dpre, int ldo, int n_out, const float* inp, int ldi, int n_in, float* dW, int ldw, float* db) {
    T.job[nj] = NmJob{dpre, inp, dW, db, ldo, n_out, ldi, n_in, ldw};
    T.start[nj] = nblocks;
    nblocks += ((n_out + 31) / 32) * ((n_in + 31) / 32);
    nj++;
  };
  const size_t RW = (size_t)R * W;
  for (int l = 0; l < NM_D; l++) {
    const float* dpre = workspace + WL.dpre + l * RW;
    if (l == 0) {
      add(dpre, W, W, acts + AL.emb, NM_EMB, in_ch, grads->w[0], in_ch, grads->b[0]);
    } else if (l == NM_SKIP + 1) {
      add(dpre, W, W, acts + AL.emb, NM_EMB, in_ch, grads->w[l], in_ch + W, grads->b[l]);
      add(dpre, W, W, acts + AL.a + (l - 1) * RW, W, W, grads->w[l] + in_ch, in_ch + W, nullptr);
    } else {
      add(dpre, W, W, acts + AL.a + (l - 1) * RW, W, W, grads->w[l], W, grads->b[l]);
    }
  }
  static const int first[NM_HEADS] = {0, 3, 6, 10, 14}, width[NM_HEADS] = {3, 3, 4, 4, 1};
  for (int h = 0; h < NM_HEADS; h++)
    if (p.hw[h])
      add(workspace + WL.dhead + first[h], 16, width[h], acts + AL.a + (NM_D - 1) * RW, W, W, grads->head_w[h], W,
          grads->head_b[h]);
  if (p.is_blender) {
    add(workspace + WL.dtn0, NM_TNH, NM_TNH, acts + AL.temb, NM_TEMB, 13, grads->tn_w0, 13, grads->tn_b0);
    add(workspace + WL.dtn1, 32, NM_TOUT, acts + AL.tnh, NM_TNH, NM_TNH, grads->tn_w1, NM_TNH, grads->tn_b1);
  }
  for (int i = nj; i < NM_JOBS; i++) { T.job[i] = T.job[0]; T.start[i] = 0x7fffffff; }
  hipLaunchKernelGGL(nm_backward_param_kernel, dim3(nblocks), dim3(256), 0, s, T, R);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
