// The 11-tap separable Gaussian window (sigma 1.5) of the image loss (csrc/loss.hip) and of the evaluation report
// (csrc/metrics.hip): tile shape, staging, the horizontal and the vertical pass.  What a kernel does to a pixel on load and what
// it makes of the windowed values is its own; everything between is here, once.
//
// 32 x 64 outputs per workgroup of 512 threads.  Both passes are register blocked: a thread produces 4 adjacent outputs from 14
// staged inputs (instead of 4 x 11).  The tall tile: 75 KB of LDS = two workgroups = four waves per SIMD (32 x 32 tiles of 256
// threads: 42 KB, three workgroups, three waves per SIMD, and 1875 workgroups = 2.4 rounds of the chip at 800 x 800 against
// 975 = 1.9 rounds here), halo overhead 1.5x instead of 1.7x.
//
// Packed fp32 throughout (v_pk_mul / v_pk_fma_f32: two fp32 operations per lane and instruction): the staged images travel as
// (x, y) PAIRS, the moments as the pairs (mu1, mu2) and (E[x^2], E[y^2]) plus the lone E[xy] — three instructions per tap and
// output instead of five multiply-adds and three products, the products of a staged pixel formed once instead of once per
// output it serves.  The kernels are bound by their vector instructions (~900 per thread), not by the LDS.  Same operations
// in the same order per element as the scalar form: bit-identical results.
#pragma once
#include <math.h>

#include "common.h"

namespace riggs {

#define SW_T 32                  // output tile: 32 columns ...
#define SW_TH 64                 // ... x 64 rows
#define SW_NT 512                // threads, 4 outputs each in either pass
#define SW_TAPS 11
#define SW_R 5                   // window radius: the apron origin of a centred (zero-padded) window is -SW_R, of a valid one 0
#define SW_A (SW_TAPS - 1)       // apron: 10 staged pixels more than outputs, either way
#define SW_S (SW_T + SW_A)       // staged columns: 42
#define SW_SH (SW_TH + SW_A)     // staged rows: 74
#define SW_PX 44                 // row pitch of the staged pairs (in pairs): rows start 16-byte aligned
#define SW_PH (SW_T + 1)         // row pitch behind the horizontal pass

typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2v pk_fma(float w, f2v a, f2v c) { return __builtin_elementwise_fma(f2v{w, w}, a, c); }
__device__ __forceinline__ float pk_fma(float w, float a, float c) { return fmaf(w, a, c); }

// gaussian(11, 1.5) as the trainer has it (loss_utils.py:33-35): a float32 tensor of the exps, divided by its float32 sum.
static inline void fill_window_f32(float* win) {
  float g[SW_TAPS], s = 0.f;
  for (int k = 0; k < SW_TAPS; k++) { g[k] = (float)exp(-(double)((k - SW_R) * (k - SW_R)) / (2.0 * 1.5 * 1.5)); s += g[k]; }
  for (int k = 0; k < SW_TAPS; k++) win[k] = g[k] / s;
}
// The same window as the evaluation packages have it: normalised to sum 1 in float64, then rounded once.
static inline void fill_window_f64(float* win) {
  double g[SW_TAPS], s = 0.0;
  for (int k = 0; k < SW_TAPS; k++) { g[k] = exp(-(double)((k - SW_R) * (k - SW_R)) / (2.0 * 1.5 * 1.5)); s += g[k]; }
  for (int k = 0; k < SW_TAPS; k++) win[k] = (float)(g[k] / s);
}

// Stages the workgroup's 74 x 42 pixels of N planes: all of the thread's global loads in flight before the first LDS write.
// `load(yy, xx, g)` reads the N values of image pixel (yy, xx) — which may lie outside the image — and `store(r, q, g)` puts
// them at staged row r, column q.  ORG: where the apron starts relative to the tile's first output (-SW_R or 0).
template <int N, int ORG, typename Load, typename Store>
__device__ __forceinline__ void sw_stage(int tid, int ty0, int tx0, Load load, Store store) {
  constexpr int NST = (SW_SH * SW_S + SW_NT - 1) / SW_NT;
  float g[NST][N];
#pragma unroll
  for (int i = 0; i < NST; i++) {
    const int e = tid + SW_NT * i, r = e / SW_S, q = e % SW_S;
    if (e < SW_SH * SW_S) load(ty0 + r + ORG, tx0 + q + ORG, g[i]);
    else
#pragma unroll
      for (int n = 0; n < N; n++) g[i][n] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < NST; i++) {
    const int e = tid + SW_NT * i, r = e / SW_S, q = e % SW_S;
    if (e < SW_SH * SW_S) store(r, q, g[i]);
  }
}

// Four adjacent outputs of one plane (pairs or scalars) from 14 inputs: accumulators start at 0, taps k = 0..10 ascending.
template <typename V>
__device__ __forceinline__ void sw_taps4(const float (&win)[SW_TAPS], const V (&in)[14], V* out) {
#pragma unroll
  for (int o = 0; o < 4; o++) {
    V acc = V(0.f);
#pragma unroll
    for (int k = 0; k < SW_TAPS; k++) acc = pk_fma(win[k], in[o + k], acc);
    out[o] = acc;
  }
}

// Horizontal pass: 74 rows x 8 groups of 4 columns over the 512 threads.  `row(r, q0)` makes columns q0..q0+3 of row r.
template <typename Row>
__device__ __forceinline__ void sw_hpass(int tid, Row row) {
  for (int e = tid; e < SW_SH * (SW_T / 4); e += SW_NT) row(e >> 3, (e & 7) * 4);
}
// ... of one plane as it is staged (row pitch P),
template <typename V, int P>
__device__ __forceinline__ void sw_row4(const float (&win)[SW_TAPS], const V (&s)[SW_SH][P], V (&h)[SW_SH][SW_PH], int r, int q0) {
  V in[14];
#pragma unroll
  for (int k = 0; k < 14; k++) in[k] = s[r][q0 + k];
  sw_taps4(win, in, &h[r][q0]);
}
// One output of the five moments, (mu1, mu2), (E[x^2], E[y^2]), E[xy], from inputs o..o+10 of the three planes.  The planes'
// taps are interleaved tap by tap: the order the kernels were tuned in (one sw_taps4 per plane compiles to coarser LDS waits).
__device__ __forceinline__ void sw_tap_moments(const float (&win)[SW_TAPS], const f2v (&a)[14], const f2v (&b)[14], const float (&c)[14], int o,
                                               f2v& m, f2v& ee, float& e12) {
  m = f2v{0.f, 0.f}; ee = f2v{0.f, 0.f}; e12 = 0.f;
#pragma unroll
  for (int k = 0; k < SW_TAPS; k++) {
    m = pk_fma(win[k], a[o + k], m);
    ee = pk_fma(win[k], b[o + k], ee);
    e12 = fmaf(win[k], c[o + k], e12);
  }
}
// ... of the five moments of a staged (x, y) plane: each pair squared and multiplied once, before the taps.
__device__ __forceinline__ void sw_row4_moments(const float (&win)[SW_TAPS], const f2v (&s_xy)[SW_SH][SW_PX], f2v (&s_m)[SW_SH][SW_PH],
                                                f2v (&s_e)[SW_SH][SW_PH], float (&s_c)[SW_SH][SW_PH], int r, int q0) {
  f2v p[14], pp[14];
  float pc[14];
#pragma unroll
  for (int k = 0; k < 14; k++) {
    p[k] = s_xy[r][q0 + k];
    pp[k] = p[k] * p[k];
    pc[k] = p[k].x * p[k].y;
  }
#pragma unroll
  for (int o = 0; o < 4; o++) {
    f2v m, ee;
    float e12;
    sw_tap_moments(win, p, pp, pc, o, m, ee, e12);
    s_m[r][q0 + o] = m; s_e[r][q0 + o] = ee; s_c[r][q0 + o] = e12;
  }
}

// Vertical pass: thread = (column lx, 4 consecutive rows ly0..ly0+3).  Of one plane,
__device__ __forceinline__ int sw_lx(int tid) { return tid & 31; }
__device__ __forceinline__ int sw_ly0(int tid) { return (tid >> 5) * 4; }
template <typename V>
__device__ __forceinline__ void sw_col4(const float (&win)[SW_TAPS], const V (&h)[SW_SH][SW_PH], int tid, V (&out)[4]) {
  V in[14];
#pragma unroll
  for (int k = 0; k < 14; k++) in[k] = h[sw_ly0(tid) + k][sw_lx(tid)];
  sw_taps4(win, in, out);
}
// ... of the five moments: the thread's 14 rows of the three planes; the kernel then takes its four outputs with sw_tap_moments,
// each followed by its epilogue (a functor for the epilogue changed the code of BOTH passes of metrics_level_kernel).
__device__ __forceinline__ void sw_col14_moments(const f2v (&s_m)[SW_SH][SW_PH], const f2v (&s_e)[SW_SH][SW_PH], const float (&s_c)[SW_SH][SW_PH],
                                                 int tid, f2v (&cm)[14], f2v (&ce)[14], float (&cc)[14]) {
  const int lx = sw_lx(tid), ly0 = sw_ly0(tid);
#pragma unroll
  for (int k = 0; k < 14; k++) { cm[k] = s_m[ly0 + k][lx]; ce[k] = s_e[ly0 + k][lx]; cc[k] = s_c[ly0 + k][lx]; }
}

}  // namespace riggs
