// Image loss of the trainer: L1 and SSIM (11x11 Gaussian window, sigma 1.5, zero padding) of a
// rendered image against the ground truth, and the gradient w.r.t. the rendered image that feeds the rasterizer backward.
//   l1_loss / ssim / _ssim   /root/reference/utils/loss_utils.py:17-18, 33-77 ;  used at /root/reference/train_rig.py:508-509
// The reference evaluates 5 grouped 11x11 conv2d (mu1, mu2, E[x^2], E[y^2], E[xy]) plus ~15 elementwise passes, and autograd
// replays them backwards.  Here: ONE forward launch (the tile and the separable window of csrc/ssim_window.h, centred: a
// 5-pixel halo of zero padding) that emits the two scalars' partial sums and three derivative maps
//   d(ssim)/d(mu1), d(ssim)/d(E[x^2]), d(ssim)/d(E[xy])
// and ONE backward launch that convolves the three maps with the (symmetric) window and combines them with the L1 sign:
//   dL/dx = g_l1 * sign(x - y) / n  +  g_ssim / n * ( G*dmu + 2 x (G*de11) + y (G*de12) ).
// Traffic: forward reads 2 images and writes 3 maps, backward reads 3 maps + 2 images and writes 1 (61 MB at 800 x 800: 8 us of
// HBM time); what the launches take is their vector instructions — see the packed forms of csrc/ssim_window.h.
#include "ssim_window.h"

namespace riggs {

struct LossArgs {
  int C, H, W;
  const float *x, *y;      // rendered image, ground truth: (C, H, W)
  float* maps;             // (3, C, H, W): dm/dmu1, dm/dE[x^2], dm/dE[xy]
  float* partial;          // [blocks][2]: sum |x - y|, sum ssim_map
  float* out2;             // [l1 mean, ssim mean]
  const float *g_l1, *g_ssim;  // backward: upstream gradients of the two scalars (device scalars)
  const float* g_loss;         // ... and of the combined loss (1 - lambda) l1 + lambda (1 - ssim)
  float lambda_dssim;
  float* dx;               // (C, H, W)
  float win[SW_TAPS];
};

__device__ __forceinline__ float ld_pad(const float* __restrict__ p, int yy, int xx, int H, int W) {
  return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? p[(size_t)yy * W + xx] : 0.f;
}

__global__ __launch_bounds__(SW_NT) void l1_ssim_forward_kernel(LossArgs a) {
  __shared__ f2v s_xy[SW_SH][SW_PX];
  __shared__ f2v s_m[SW_SH][SW_PH], s_e[SW_SH][SW_PH];  // after the horizontal pass: (mu1, mu2), (E[x^2], E[y^2])
  __shared__ float s_c[SW_SH][SW_PH];                   // ... E[xy]
  __shared__ float s_red[2][SW_NT / 64];
  const int c = blockIdx.z, tx0 = blockIdx.x * SW_T, ty0 = blockIdx.y * SW_TH;
  const int tid = threadIdx.x;
  const float* X = a.x + (size_t)c * a.H * a.W;
  const float* Y = a.y + (size_t)c * a.H * a.W;
  sw_stage<2, -SW_R>(
      tid, ty0, tx0, [&](int yy, int xx, float(&g)[2]) { g[0] = ld_pad(X, yy, xx, a.H, a.W); g[1] = ld_pad(Y, yy, xx, a.H, a.W); },
      [&](int r, int q, const float(&g)[2]) { s_xy[r][q] = f2v{g[0], g[1]}; });
  __syncthreads();
  float win[SW_TAPS];
#pragma unroll
  for (int k = 0; k < SW_TAPS; k++) win[k] = a.win[k];
  sw_hpass(tid, [&](int r, int q0) { sw_row4_moments(win, s_xy, s_m, s_e, s_c, r, q0); });
  __syncthreads();
  f2v mo_m[4], mo_e[4];
  float mo_c[4];
  {
    f2v cm[14], ce[14];
    float cc[14];
    sw_col14_moments(s_m, s_e, s_c, tid, cm, ce, cc);
#pragma unroll
    for (int o = 0; o < 4; o++) sw_tap_moments(win, cm, ce, cc, o, mo_m[o], mo_e[o], mo_c[o]);
  }
  const int lx = sw_lx(tid), ly0 = sw_ly0(tid);
  float ssim_sum = 0.f, ad_sum = 0.f;
  const size_t plane = (size_t)a.C * a.H * a.W;
  const int px = tx0 + lx;
#pragma unroll
  for (int o = 0; o < 4; o++) {
    const int py = ty0 + ly0 + o;
    if (px < a.W && py < a.H) {
      const float m1 = mo_m[o].x, m2 = mo_m[o].y, e11 = mo_e[o].x, e22 = mo_e[o].y, e12 = mo_c[o];
      const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;  // loss_utils.py:67-68
      const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
      const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
      const float A = 2.f * mu12 + C1, B = 2.f * s12 + C2, Cc = mu1_sq + mu2_sq + C1, D = s1 + s2 + C2;
      const float inv = 1.0f / (Cc * D);
      const float ssim = A * B * inv;
      const size_t idx = ((size_t)c * a.H + py) * a.W + px;
      a.maps[idx] = 2.f * m2 * (B - A) * inv - ssim * 2.f * m1 * (D - Cc) * inv;  // d/dmu1 (through sigma1^2, sigma12 too)
      a.maps[plane + idx] = -ssim / D;                                            // d/dE[x^2]
      a.maps[2 * plane + idx] = 2.f * A * inv;                                    // d/dE[xy]
      ssim_sum += ssim;
      const f2v ctr = s_xy[ly0 + o + SW_R][lx + SW_R];
      ad_sum += fabsf(ctr.x - ctr.y);
    }
  }
  const float ad = wave_sum(ad_sum), ss = wave_sum(ssim_sum);
  if ((tid & 63) == 63) { s_red[0][tid >> 6] = ad; s_red[1][tid >> 6] = ss; }
  __syncthreads();
  if (tid == 0) {
    const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.partial[2 * b] = ((s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3])) + ((s_red[0][4] + s_red[0][5]) + (s_red[0][6] + s_red[0][7]));
    a.partial[2 * b + 1] = ((s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3])) + ((s_red[1][4] + s_red[1][5]) + (s_red[1][6] + s_red[1][7]));
  }
}

// fixed-order sum of the per-workgroup partials (deterministic), / n
__global__ __launch_bounds__(1024) void l1_ssim_finish_kernel(int n_blocks, const float* __restrict__ partial, double inv_n,
                                                              float lambda_dssim, float* __restrict__ out2) {
  __shared__ double s_w[2][16];
  double s0 = 0.0, s1 = 0.0;
  for (int i = threadIdx.x; i < n_blocks; i += 1024) { s0 += (double)partial[2 * i]; s1 += (double)partial[2 * i + 1]; }
  s0 = wave_sum_f64(s0); s1 = wave_sum_f64(s1);
  if ((threadIdx.x & 63) == 0) { s_w[0][threadIdx.x >> 6] = s0; s_w[1][threadIdx.x >> 6] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0.0, t1 = 0.0;
    for (int w = 0; w < 16; w++) { t0 += s_w[0][w]; t1 += s_w[1][w]; }
    const float l1 = (float)(t0 * inv_n), ss = (float)(t1 * inv_n);
    out2[0] = l1; out2[1] = ss;
    out2[2] = (1.0f - lambda_dssim) * l1 + lambda_dssim * (1.0f - ss);  // train_rig.py:509
  }
}

__global__ __launch_bounds__(SW_NT) void l1_ssim_backward_kernel(LossArgs a) {
  // (packed like the forward: the maps d/dmu1 and d/dE[x^2] travel as a pair, d/dE[xy] alone)
  __shared__ f2v s_ab[SW_SH][SW_PX];
  __shared__ float s_cc[SW_SH][SW_S + 1];
  __shared__ f2v s_hab[SW_SH][SW_PH];
  __shared__ float s_hc[SW_SH][SW_PH];
  const int c = blockIdx.z, tx0 = blockIdx.x * SW_T, ty0 = blockIdx.y * SW_TH;
  const int tid = threadIdx.x;
  const size_t plane = (size_t)a.C * a.H * a.W, chan = (size_t)c * a.H * a.W;
  sw_stage<3, -SW_R>(
      tid, ty0, tx0,
      [&](int yy, int xx, float(&g)[3]) {
        g[0] = ld_pad(a.maps + chan, yy, xx, a.H, a.W);
        g[1] = ld_pad(a.maps + plane + chan, yy, xx, a.H, a.W);
        g[2] = ld_pad(a.maps + 2 * plane + chan, yy, xx, a.H, a.W);
      },
      [&](int r, int q, const float(&g)[3]) { s_ab[r][q] = f2v{g[0], g[1]}; s_cc[r][q] = g[2]; });
  // (this thread's four pixels of both images: asked for here, used behind the two passes)
  const int lx = sw_lx(tid), ly0 = sw_ly0(tid);
  const int px = tx0 + lx;
  float xs[4], ys[4];
#pragma unroll
  for (int o = 0; o < 4; o++) {
    const int py = ty0 + ly0 + o;
    const bool in = px < a.W && py < a.H;
    const size_t idx = chan + (size_t)py * a.W + px;
    xs[o] = in ? a.x[idx] : 0.f;
    ys[o] = in ? a.y[idx] : 0.f;
  }
  __syncthreads();
  float win[SW_TAPS];
#pragma unroll
  for (int k = 0; k < SW_TAPS; k++) win[k] = a.win[k];
  sw_hpass(tid, [&](int r, int q0) { sw_row4(win, s_ab, s_hab, r, q0); sw_row4(win, s_cc, s_hc, r, q0); });
  __syncthreads();
  f2v cv_ab[4];
  float cv_c[4];
  sw_col4(win, s_hab, tid, cv_ab);
  sw_col4(win, s_hc, tid, cv_c);
  const float inv_n = 1.0f / (float)plane;
  const float gt_ = a.g_loss ? a.g_loss[0] : 0.f;
  const float gl = (a.g_l1 ? a.g_l1[0] : 0.f) + (1.0f - a.lambda_dssim) * gt_;
  const float gs = (a.g_ssim ? a.g_ssim[0] : 0.f) - a.lambda_dssim * gt_;
#pragma unroll
  for (int o = 0; o < 4; o++) {
    const int py = ty0 + ly0 + o;
    if (px < a.W && py < a.H) {
      const size_t idx = chan + (size_t)py * a.W + px;
      const float x = xs[o], y = ys[o];
      const float d = x - y;
      const float sgn = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);  // torch.abs backward: sign(0) = 0
      a.dx[idx] = gl * sgn * inv_n + gs * inv_n * (cv_ab[o].x + 2.f * x * cv_ab[o].y + y * cv_c[o]);
    }
  }
}

}  // namespace riggs

using namespace riggs;

extern "C" {

static size_t ls_blocks(int C, int H, int W) { return (size_t)C * ((H + SW_TH - 1) / SW_TH) * ((W + SW_T - 1) / SW_T); }

size_t riggs_l1_ssim_state_floats(int32_t C, int32_t H, int32_t W) {
  return 3 * (size_t)C * H * W + 2 * ls_blocks(C, H, W);
}

int riggs_l1_ssim_forward(int32_t C, int32_t H, int32_t W, const float* image, const float* gt, float lambda_dssim,
                          float* state, float* out2, riggs_stream stream) {
  RIGGS_REQUIRE(C >= 1 && H >= 1 && W >= 1 && C <= 65535, "bad image shape");
  RIGGS_REQUIRE(image && gt && state && out2, "NULL buffer");
  LossArgs a;
  memset(&a, 0, sizeof(a));
  a.C = C; a.H = H; a.W = W; a.x = image; a.y = gt;
  a.maps = state; a.partial = state + 3 * (size_t)C * H * W; a.out2 = out2;
  fill_window_f32(a.win);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((W + SW_T - 1) / SW_T, (H + SW_TH - 1) / SW_TH, C);
  {
    ProfScope ps(PROF_LOSS_FWD, s);
    hipLaunchKernelGGL(l1_ssim_forward_kernel, grid, dim3(SW_NT), 0, s, a);
    hipLaunchKernelGGL(l1_ssim_finish_kernel, dim3(1), dim3(1024), 0, s, (int)ls_blocks(C, H, W), a.partial,
                       1.0 / ((double)C * H * W), lambda_dssim, out2);
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_l1_ssim_backward(int32_t C, int32_t H, int32_t W, const float* image, const float* gt, const float* state,
                           float lambda_dssim, const float* g_l1, const float* g_ssim, const float* g_loss,
                           float* dL_dimage, riggs_stream stream) {
  RIGGS_REQUIRE(C >= 1 && H >= 1 && W >= 1 && C <= 65535, "bad image shape");
  RIGGS_REQUIRE(image && gt && state && dL_dimage, "NULL buffer");
  LossArgs a;
  memset(&a, 0, sizeof(a));
  a.C = C; a.H = H; a.W = W; a.x = image; a.y = gt;
  a.maps = const_cast<float*>(state); a.g_l1 = g_l1; a.g_ssim = g_ssim; a.g_loss = g_loss; a.lambda_dssim = lambda_dssim;
  a.dx = dL_dimage;
  fill_window_f32(a.win);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((W + SW_T - 1) / SW_T, (H + SW_TH - 1) / SW_TH, C);
  {
    ProfScope ps(PROF_LOSS_BWD, s);
    hipLaunchKernelGGL(l1_ssim_backward_kernel, grid, dim3(SW_NT), 0, s, a);
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
