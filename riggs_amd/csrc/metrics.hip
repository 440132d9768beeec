// Evaluation report: L1, PSNR, SSIM (piq.ssim) and MS-SSIM (pytorch_msssim.ms_ssim) of B rendered frames against their ground
// truth — the numbers of skeleton_training_report (train_utils.py:56-243) and render_set (render_rig.py:111-218).
// Both SSIMs are the same per-level computation: an 11-tap separable Gaussian (sigma 1.5) over the five moments
//   mu1, mu2, E[x^2], E[y^2], E[xy]
// with a VALID window (output (i, j) covers inputs i..i+10, j..j+10 — not the zero padding of the training loss, csrc/loss.hip),
// reduced to two means per (frame, channel):
//   cs_map = (2 s12 + C2) / (s1 + s2 + C2),   ssim_map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs_map.
// The reference's packages issue ~150 small launches per frame for this; here a batch of frames costs
//   level 0 | pool | level 1 | pool | level 2 | pool | level 3 | pool | level 4 | [pool by f | piq level] | finalise
// = at most 12 launches whatever B is.  The 2x2 pool is a launch of its own, not folded into the level kernel: a folded pool
// needs the pixel left of / above the tile when the size is odd, and the pyramid (1/3 of the input) is not where the time goes.
// Traffic at (3, 800, 800): 2 x 7.7 MB read by level 0 and again by the pools, 2.6 MB of pyramid written and read back:
// ~40 MB per frame, 8 us of HBM time against 33 us per frame measured at B = 20: not memory-bound (the instruction mix is the
// loss kernel's, which was bound by its vector instructions).
// Sums: every workgroup adds its float32 map values in float64 and stores four float64 partials; the finalise kernel adds a
// (frame, channel)'s partials in a fixed order.  No float atomics: a frame's numbers do not depend on B, on its neighbours in the
// batch or on the run.
#include "metrics.h"
#include "ssim_window.h"

namespace riggs {

#define MT_PLANES_PER_LAUNCH 65535
// The variances and the covariance do not change when a constant is taken off both images; E[x^2] - mu^2 loses the fewer bits the
// smaller E[x^2] is.  Images live in [0, 1]: the moments are formed of x - 0.5 and y - 0.5 (an exact subtraction for x >= 0.25),
// which cut the deviation from the float64 definition about tenfold on the test images; mu = (G*(x - 0.5)) + 0.5 for the
// luminance term.  L1 and the squared error are formed of the unshifted values.
#define MT_SHIFT 0.5f

struct LevelArgs {
  int h, w;         // this level's image size
  int plane0;       // first plane (b * C + c) of this launch
  int clamp;        // clamp both inputs to [0, 1] on load (level 0 of a clamp=1 call; later levels are made from clamped values)
  int first;        // level 0: also sum |x - y| and (x - y)^2, every input pixel by the workgroup that owns it
  const float *x, *y;  // (planes, h, w)
  double* partial;     // [plane][workgroup][4]: sum ssim_map, sum cs_map, sum |x - y|, sum (x - y)^2
  float win[SW_TAPS];
};

__global__ __launch_bounds__(SW_NT) void metrics_level_kernel(LevelArgs a) {
  __shared__ f2v s_xy[SW_SH][SW_PX];
  __shared__ f2v s_m[SW_SH][SW_PH], s_e[SW_SH][SW_PH];
  __shared__ float s_c[SW_SH][SW_PH];
  __shared__ double s_red[4][SW_NT / 64];
  const int tx0 = blockIdx.x * SW_T, ty0 = blockIdx.y * SW_TH;
  const int tid = threadIdx.x;
  // (read once, here: when the staging functors read them through the captured argument struct, THIS kernel loaded them again
  // behind the barriers and its vertical pass waited for the LDS more coarsely; the loss kernels capture theirs without such an effect)
  const int h = a.h, w = a.w, clamp = a.clamp, first = a.first;
  const size_t plane = (size_t)a.plane0 + blockIdx.z;
  const float* X = a.x + plane * a.h * a.w;
  const float* Y = a.y + plane * a.h * a.w;
  // A workgroup owns the input pixels under its 32 x 64 outputs; the last one of a row / column of workgroups also owns the
  // apron, which ends at or before the image's edge there (the outputs end 10 pixels before it).
  const bool last_x = blockIdx.x == gridDim.x - 1, last_y = blockIdx.y == gridDim.y - 1;
  double ad_sum = 0.0, sq_sum = 0.0;
  sw_stage<2, 0>(
      tid, ty0, tx0,
      [&](int yy, int xx, float(&g)[2]) {
        const bool in = yy < h && xx < w;
        const size_t idx = (size_t)yy * w + xx;
        g[0] = in ? X[idx] : 0.f;
        g[1] = in ? Y[idx] : 0.f;
      },
      [&](int r, int q, const float(&g)[2]) {
        float vx = g[0], vy = g[1];
        if (clamp) { vx = fminf(fmaxf(vx, 0.f), 1.f); vy = fminf(fmaxf(vy, 0.f), 1.f); }
        s_xy[r][q] = f2v{vx - MT_SHIFT, vy - MT_SHIFT};
        const bool owned = ty0 + r < h && tx0 + q < w && (r < SW_TH || last_y) && (q < SW_T || last_x);
        if (first && owned) {
          const float d = vx - vy, d2 = d * d;  // float32 difference and square, float64 sums
          ad_sum += (double)fabsf(d);
          sq_sum += (double)d2;
        }
      });
  __syncthreads();
  float win[SW_TAPS];
#pragma unroll
  for (int k = 0; k < SW_TAPS; k++) win[k] = a.win[k];
  sw_hpass(tid, [&](int r, int q0) { sw_row4_moments(win, s_xy, s_m, s_e, s_c, r, q0); });
  __syncthreads();
  double ssim_sum = 0.0, cs_sum = 0.0;
  const int px = tx0 + sw_lx(tid);
  f2v cm[14], ce[14];
  float cc[14];
  sw_col14_moments(s_m, s_e, s_c, tid, cm, ce, cc);
#pragma unroll
  for (int o = 0; o < 4; o++) {
    f2v m, ee;
    float e12;
    sw_tap_moments(win, cm, ce, cc, o, m, ee, e12);
    const int py = ty0 + sw_ly0(tid) + o;
    if (px < w - SW_A && py < h - SW_A) {
      const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
      const float s1 = ee.x - m.x * m.x, s2 = ee.y - m.y * m.y, s12 = e12 - m.x * m.y;  // (of the shifted images)
      const float m1 = m.x + MT_SHIFT, m2 = m.y + MT_SHIFT;
      const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
      const float cs = (2.f * s12 + C2) / (s1 + s2 + C2);
      const float ss = (2.f * mu12 + C1) / (mu1_sq + mu2_sq + C1) * cs;
      ssim_sum += (double)ss;
      cs_sum += (double)cs;
    }
  }
  const double r0 = wave_sum_f64(ssim_sum), r1 = wave_sum_f64(cs_sum), r2 = wave_sum_f64(ad_sum), r3 = wave_sum_f64(sq_sum);
  if ((tid & 63) == 0) { s_red[0][tid >> 6] = r0; s_red[1][tid >> 6] = r1; s_red[2][tid >> 6] = r2; s_red[3][tid >> 6] = r3; }
  __syncthreads();
  if (tid < 4) {
    double t = 0.0;
    for (int wv = 0; wv < SW_NT / 64; wv++) t += s_red[tid][wv];
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x, n_wg = (size_t)gridDim.x * gridDim.y;
    a.partial[(plane * n_wg + wg) * 4 + tid] = t;
  }
}

// Mean pooling, kernel k, stride k, `ph` / `pw` zeros in front of the rows / columns that count in the divisor
// (avg_pool2d(count_include_pad=True)); windows that the image does not fill are dropped: oh = (h + ph) / k, ow = (w + pw) / k.
struct PoolArgs {
  int h, w, oh, ow, k, ph, pw, plane0, clamp;
  size_t planes;           // the destination holds x's planes, then y's
  const float *x, *y;
  float* dst;
};

__global__ __launch_bounds__(256) void metrics_pool_kernel(PoolArgs a) {
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x, on = (size_t)a.oh * a.ow;
  if (o >= on) return;
  const int oi = (int)(o / a.ow), oj = (int)(o % a.ow);
  const size_t plane = (size_t)a.plane0 + blockIdx.y;
  const float* X = a.x + plane * a.h * a.w;
  const float* Y = a.y + plane * a.h * a.w;
  float sx = 0.f, sy = 0.f;
  for (int di = 0; di < a.k; di++) {
    const int ii = oi * a.k - a.ph + di;
    for (int dj = 0; dj < a.k; dj++) {
      const int jj = oj * a.k - a.pw + dj;
      float vx = 0.f, vy = 0.f;
      if (ii >= 0 && jj >= 0) { vx = X[(size_t)ii * a.w + jj]; vy = Y[(size_t)ii * a.w + jj]; }
      if (a.clamp) { vx = fminf(fmaxf(vx, 0.f), 1.f); vy = fminf(fmaxf(vy, 0.f), 1.f); }
      sx += vx; sy += vy;
    }
  }
  const float div = (float)(a.k * a.k);
  a.dst[plane * on + o] = sx / div;
  a.dst[(a.planes + plane) * on + o] = sy / div;
}

struct FinalArgs {
  int C, want_ms;
  int active[MT_LEVELS];     // the level was computed by this call
  int n_wg[MT_LEVELS];       // partials per plane
  size_t part[MT_LEVELS];    // offset in doubles
  double count[MT_LEVELS];   // valid outputs per plane: (h - 10) (w - 10)
  double pixels;             // H * W
  const double* partial;
  float* out;                // (B, 4): l1, psnr, ssim, ms_ssim
  float* levels;             // (B, 6, C, 2) or NULL
};

#define MT_FIN_NT 256

// One workgroup per frame.  Each (level, channel): thread t adds partials t, t + 256, ... , then the 256 sums are added in a
// fixed order — float64 throughout.
__global__ __launch_bounds__(MT_FIN_NT) void metrics_finalise_kernel(FinalArgs a) {
  __shared__ double s_w[4][MT_FIN_NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double wt[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  const double nan = __builtin_nan("");
  double ad_tot = 0.0, sq_tot = 0.0, ssim_tot = 0.0, ms_tot = 0.0;  // (thread 0's)
  for (int c = 0; c < a.C; c++) {
    const size_t plane = (size_t)b * a.C + c;
    double prod = 1.0;
    for (int l = 0; l < MT_LEVELS; l++) {
      double mean_ss = nan, mean_cs = nan;
      if (a.active[l]) {  // (uniform over the workgroup)
        const double* p = a.partial + a.part[l] + plane * a.n_wg[l] * 4;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < a.n_wg[l]; i += MT_FIN_NT)
          for (int k = 0; k < 4; k++) v[k] += p[(size_t)i * 4 + k];
        for (int k = 0; k < 4; k++) v[k] = wave_sum_f64(v[k]);
        __syncthreads();  // (the previous round's reads of s_w)
        if ((tid & 63) == 0)
          for (int k = 0; k < 4; k++) s_w[k][tid >> 6] = v[k];
        __syncthreads();
        if (tid == 0) {
          for (int k = 0; k < 4; k++) {
            v[k] = 0.0;
            for (int wv = 0; wv < MT_FIN_NT / 64; wv++) v[k] += s_w[k][wv];
          }
          mean_ss = v[0] / a.count[l];
          mean_cs = v[1] / a.count[l];
          if (l == 0) { ad_tot += v[2]; sq_tot += v[3]; }
          if (l < 4) prod *= pow(fmax(mean_cs, 0.0), wt[l]);        // relu(cs_c) ^ wt_l
          else if (l == 4) prod *= pow(fmax(mean_ss, 0.0), wt[4]);  // relu(ssim_c) of the last level
          else ssim_tot += mean_ss;
        }
      }
      if (tid == 0 && a.levels) {
        float* q = a.levels + (((size_t)b * MT_LEVELS + l) * a.C + c) * 2;
        q[0] = (float)mean_ss; q[1] = (float)mean_cs;
      }
    }
    if (tid == 0) ms_tot += prod;
  }
  if (tid == 0) {
    const double n = a.pixels * a.C;
    const double mse = sq_tot / n;
    float* o = a.out + (size_t)b * 4;
    o[0] = (float)(ad_tot / n);
    o[1] = (float)(20.0 * log10(1.0 / sqrt(mse)));  // image_utils.py:30-32; identical images: inf
    o[2] = (float)(ssim_tot / a.C);
    o[3] = a.want_ms ? (float)(ms_tot / a.C) : (float)nan;
  }
}

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

MetricsPlan metrics_plan(int B, int C, int H, int W) {
  MetricsPlan p;
  memset(&p, 0, sizeof(p));
  const int m = H < W ? H : W;
  const size_t planes = (size_t)B * C;
  // Python's round(m / 256): half to even (640 -> 2, 896 -> 4)
  {
    const int q = m / 256, r = m % 256;
    int f = q + (r > 128 || (r == 128 && (q & 1)) ? 1 : 0);
    p.f = f < 1 ? 1 : f;
  }
  p.ms = m > 160;
  p.h[0] = H; p.w[0] = W;
  for (int l = 1; l < 5; l++) {
    p.h[l] = p.ms ? (p.h[l - 1] + 1) / 2 : 0;  // pool by 2 with (h % 2) zeros in front: ceil(h / 2)
    p.w[l] = p.ms ? (p.w[l - 1] + 1) / 2 : 0;
  }
  p.h[5] = H / p.f; p.w[5] = W / p.f;
  size_t d = 0;
  for (int l = 0; l < MT_LEVELS; l++) {
    const bool runs = p.h[l] >= SW_TAPS && p.w[l] >= SW_TAPS;
    p.tx[l] = runs ? ceil_div(p.w[l] - SW_A, SW_T) : 0;
    p.ty[l] = runs ? ceil_div(p.h[l] - SW_A, SW_TH) : 0;
    if (l == 5 && p.f == 1) { p.part[5] = p.part[0]; break; }  // the piq level is level 0
    p.part[l] = d;
    d += planes * p.tx[l] * p.ty[l] * 4;
  }
  size_t fl = 2 * d;  // (the float64 partials lead the workspace: 8-byte aligned when the workspace is)
  for (int l = 1; l < MT_LEVELS; l++) {
    if (l == 5 && p.f == 1) break;
    p.img[l] = fl;
    fl += 2 * planes * (size_t)p.h[l] * p.w[l];
  }
  p.total_floats = fl;
  return p;
}

int launch_image_metrics(const MetricsPlan& p, int B, int C, int H, int W, const float* x, const float* y, int clamp, int want_ms,
                         float* out, float* levels, float* workspace, hipStream_t s) {
  const size_t planes = (size_t)B * C;
  double* partial = (double*)workspace;
  auto level = [&](int l, const float* lx, const float* ly, int cl) {
    LevelArgs a;
    a.h = p.h[l]; a.w = p.w[l]; a.clamp = cl; a.first = l == 0; a.x = lx; a.y = ly; a.partial = partial + p.part[l];
    fill_window_f64(a.win);
    for (size_t p0 = 0; p0 < planes; p0 += MT_PLANES_PER_LAUNCH) {
      const size_t n = planes - p0 < MT_PLANES_PER_LAUNCH ? planes - p0 : MT_PLANES_PER_LAUNCH;
      a.plane0 = (int)p0;
      hipLaunchKernelGGL(metrics_level_kernel, dim3(p.tx[l], p.ty[l], (unsigned)n), dim3(SW_NT), 0, s, a);
    }
  };
  auto pool = [&](int from, int to, int k, int ph, int pw, const float* sx, const float* sy, int cl) {
    PoolArgs a;
    a.h = p.h[from]; a.w = p.w[from]; a.oh = p.h[to]; a.ow = p.w[to]; a.k = k; a.ph = ph; a.pw = pw; a.clamp = cl;
    a.planes = planes; a.x = sx; a.y = sy; a.dst = workspace + p.img[to];
    const size_t on = (size_t)a.oh * a.ow;
    for (size_t p0 = 0; p0 < planes; p0 += MT_PLANES_PER_LAUNCH) {
      const size_t n = planes - p0 < MT_PLANES_PER_LAUNCH ? planes - p0 : MT_PLANES_PER_LAUNCH;
      a.plane0 = (int)p0;
      hipLaunchKernelGGL(metrics_pool_kernel, dim3((unsigned)((on + 255) / 256), (unsigned)n), dim3(256), 0, s, a);
    }
  };
  auto img_x = [&](int l) { return l == 0 ? x : workspace + p.img[l]; };
  auto img_y = [&](int l) { return l == 0 ? y : workspace + p.img[l] + planes * (size_t)p.h[l] * p.w[l]; };
  FinalArgs fa;
  memset(&fa, 0, sizeof(fa));
  level(0, x, y, clamp);
  fa.active[0] = 1;
  if (want_ms)
    for (int l = 1; l < 5; l++) {
      pool(l - 1, l, 2, p.h[l - 1] % 2, p.w[l - 1] % 2, img_x(l - 1), img_y(l - 1), l == 1 ? clamp : 0);
      level(l, img_x(l), img_y(l), 0);
      fa.active[l] = 1;
    }
  if (p.f > 1) {
    pool(0, 5, p.f, 0, 0, x, y, clamp);
    level(5, img_x(5), img_y(5), 0);
  }
  fa.active[5] = 1;
  fa.C = C; fa.want_ms = want_ms; fa.pixels = (double)H * W; fa.partial = partial; fa.out = out; fa.levels = levels;
  for (int l = 0; l < MT_LEVELS; l++) {
    fa.n_wg[l] = p.tx[l] * p.ty[l];
    fa.part[l] = p.part[l];
    fa.count[l] = (double)(p.h[l] - SW_A) * (double)(p.w[l] - SW_A);
  }
  if (p.f == 1) fa.n_wg[5] = fa.n_wg[0];
  hipLaunchKernelGGL(metrics_finalise_kernel, dim3(B), dim3(MT_FIN_NT), 0, s, fa);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace riggs
