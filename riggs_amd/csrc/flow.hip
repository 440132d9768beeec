// Optical-flow supervision of a stage-1 iteration (train_gui.py:1078-1121): the per-Gaussian flow colours that
// gaussian_renderer.render_flow (gaussian_renderer/__init__.py:186-202) hands to the rasterizer, and the masked, weighted L1
// between the rendered motion and the RAFT flow (train_gui.py:1101-1120), each with its backward.
//
// Colours: the reference builds them from ~15 element-wise torch ops and three cats over all N Gaussians,
//   p1 = x + d_xyz1, p2 = x + d_xyz2 (x detached), u_k = ([p_k, 1] . F_k).xyz / ([p_k, 1] . F_k).w,
//   colour = (u2.x - u1.x, u2.y - u1.y, motion_mask)
// and autograd replays them.  Here: ONE launch forward (40 B read + 12 B written per Gaussian) and ONE launch backward
// (52 B + 28 B) that recomputes the projections; nothing is saved.  One thread per Gaussian; the (N, 3) streams go through LDS
// so that every global access is a run of consecutive dwords.  The two matrices are read from their device tensors with
// uniform (scalar) loads.
//
// Loss: ~20 element-wise torch ops over the image become one forward launch (+ the fixed-order sum of its per-workgroup
// partials) and one backward launch.  The weight w is the reference's to rounding (a few ulps: the mean is a product with
// 1 / C and the cosines' arguments a product with a rounded pi / 2 here); c = flow / (W, H) * 2 and fl(w c) - fl(w m) are the
// reference's operations one by one (FP contraction off: no fused multiply-subtract), so that for a given w the sign of a
// term is decided as the reference decides it, and forward and backward of this file decide it alike.
#include "common.h"

namespace riggs {

#define FC_NT 256  // Gaussians (= threads) per workgroup

// (rows, 3) stream -> LDS, coalesced: thread t moves dwords t, t + 256, t + 512 of the workgroup's 768
__device__ __forceinline__ void rows3_in(const float* __restrict__ src, size_t base, size_t total, float* lds) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const size_t e = base + threadIdx.x + FC_NT * k;
    lds[threadIdx.x + FC_NT * k] = (src && e < total) ? src[e] : 0.f;
  }
}
__device__ __forceinline__ void rows3_out(float* __restrict__ dst, size_t base, size_t total, const float* lds) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const size_t e = base + threadIdx.x + FC_NT * k;
    if (e < total) dst[e] = lds[threadIdx.x + FC_NT * k];
  }
}

// h = [p, 1] . F with F a row-major (4, 4) in row-vector convention: h_j = p_x F[0][j] + p_y F[1][j] + p_z F[2][j] + F[3][j]
struct Proj { float u[2], w; };
__device__ __forceinline__ Proj project(const float* __restrict__ F, float x, float y, float z) {
  const float hx = ((x * F[0] + y * F[4]) + z * F[8]) + F[12];
  const float hy = ((x * F[1] + y * F[5]) + z * F[9]) + F[13];
  const float hw = ((x * F[3] + y * F[7]) + z * F[11]) + F[15];
  Proj r;
  r.u[0] = hx / hw; r.u[1] = hy / hw; r.w = hw;  // plain division: no + 1e-7 (gaussian_renderer/__init__.py:193, :197)
  return r;
}

__device__ __forceinline__ float flow_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

struct FlowColorArgs {
  int N;
  const float *xyz, *d1, *d2;  // (N, 3); d1 / d2 may be NULL (a residual of 0.0)
  const float *F1, *F2;        // device (4, 4)
  const float* logit;          // motion-mask logit of Gaussian n at logit[n * logit_stride]; NULL: mask = 1
  long long logit_stride;
  float* colour;               // forward out (N, 3)
  const float* g_colour;       // backward in (N, 3)
  float *g_d1, *g_d2, *g_logit;  // backward out (N, 3), (N, 3), (N); each may be NULL
};

__global__ __launch_bounds__(FC_NT) void flow_colors_forward_kernel(FlowColorArgs a) {
  __shared__ float s_x[3 * FC_NT], s_1[3 * FC_NT], s_2[3 * FC_NT];
  const size_t base = (size_t)blockIdx.x * (3 * FC_NT), total = (size_t)a.N * 3;
  rows3_in(a.xyz, base, total, s_x);
  rows3_in(a.d1, base, total, s_1);
  rows3_in(a.d2, base, total, s_2);
  const int n = blockIdx.x * FC_NT + threadIdx.x, t3 = 3 * threadIdx.x;
  const float m = (a.logit && n < a.N) ? flow_sigmoid(a.logit[(long long)n * a.logit_stride]) : 1.0f;
  __syncthreads();
  const float x = s_x[t3], y = s_x[t3 + 1], z = s_x[t3 + 2];
  const Proj p1 = project(a.F1, x + s_1[t3], y + s_1[t3 + 1], z + s_1[t3 + 2]);
  const Proj p2 = project(a.F2, x + s_2[t3], y + s_2[t3 + 1], z + s_2[t3 + 2]);
  __syncthreads();
  s_x[t3] = p2.u[0] - p1.u[0]; s_x[t3 + 1] = p2.u[1] - p1.u[1]; s_x[t3 + 2] = m;
  __syncthreads();
  rows3_out(a.colour, base, total, s_x);
}

// dL/dp of one camera from (gx, gy) = dL/du.xy: dL/dh = (gx / w, gy / w, ., -(gx u_x + gy u_y) / w), dL/dp_i = sum_j F[i][j] dL/dh_j
__device__ __forceinline__ void project_backward(const float* __restrict__ F, const Proj& p, float gx, float gy, float* g) {
  const float ghx = gx / p.w, ghy = gy / p.w, ghw = -((gx * p.u[0] + gy * p.u[1]) / p.w);
#pragma unroll
  for (int i = 0; i < 3; i++) g[i] = (F[4 * i] * ghx + F[4 * i + 1] * ghy) + F[4 * i + 3] * ghw;
}

__global__ __launch_bounds__(FC_NT) void flow_colors_backward_kernel(FlowColorArgs a) {
  __shared__ float s_x[3 * FC_NT], s_1[3 * FC_NT], s_2[3 * FC_NT], s_g[3 * FC_NT];
  const size_t base = (size_t)blockIdx.x * (3 * FC_NT), total = (size_t)a.N * 3;
  rows3_in(a.xyz, base, total, s_x);
  rows3_in(a.d1, base, total, s_1);
  rows3_in(a.d2, base, total, s_2);
  rows3_in(a.g_colour, base, total, s_g);
  const int n = blockIdx.x * FC_NT + threadIdx.x, t3 = 3 * threadIdx.x;
  __syncthreads();
  const float gx = s_g[t3], gy = s_g[t3 + 1], gm = s_g[t3 + 2];
  float g1[3] = {0.f, 0.f, 0.f}, g2[3] = {0.f, 0.f, 0.f};
  // A row without an incoming flow gradient — every culled Gaussian, every Gaussian that reached no pixel — gets exact
  // zeros: the reference's 0 * (1 / w) would be NaN where w = 0 (a point on the camera plane of the paired frame).
  if (gx != 0.f || gy != 0.f) {
    const float x = s_x[t3], y = s_x[t3 + 1], z = s_x[t3 + 2];
    const Proj p1 = project(a.F1, x + s_1[t3], y + s_1[t3 + 1], z + s_1[t3 + 2]);
    const Proj p2 = project(a.F2, x + s_2[t3], y + s_2[t3 + 1], z + s_2[t3 + 2]);
    project_backward(a.F1, p1, -gx, -gy, g1);
    project_backward(a.F2, p2, gx, gy, g2);
  }
  if (a.g_logit && n < a.N) {
    float gl = 0.f;
    if (gm != 0.f && a.logit) {
      const float m = flow_sigmoid(a.logit[(long long)n * a.logit_stride]);
      gl = gm * (m * (1.0f - m));
    }
    a.g_logit[n] = gl;
  }
  __syncthreads();
  s_1[t3] = g1[0]; s_1[t3 + 1] = g1[1]; s_1[t3 + 2] = g1[2];
  s_2[t3] = g2[0]; s_2[t3 + 1] = g2[1]; s_2[t3 + 2] = g2[2];
  __syncthreads();
  if (a.g_d1) rows3_out(a.g_d1, base, total, s_1);
  if (a.g_d2) rows3_out(a.g_d2, base, total, s_2);
}

// ---- the loss --------------------------------------------------------------------------------------------------------------
#define FL_NT 256
#define FL_PX 4  // pixels per thread: a workgroup covers 1024 consecutive pixels

struct FlowLossArgs {
  int C, H, W, MC;             // image channels, size, channels of `masks`
  const float *image, *gt;     // (C, H, W)
  const float* motion;         // (3, H, W): planes 0 and 1 are read
  const float* alpha;          // (H, W)
  const float* flow;           // (H, W, 2), RAFT pixels
  const float* masks;          // (H, W, MC), channels 0 and 1 are read
  const float *fid1_dev, *fid2_dev;  // device scalars, or NULL: the values below
  float fid1, fid2;
  float* weight;               // (H, W)
  float* partial;              // [workgroups]
  float* loss;                 // device scalar
  const float* g_loss;         // backward: upstream gradient (device scalar)
  float* g_motion;             // (3, H, W)
};

#define FL_HALF_PI 1.57079632679489661923f

__device__ __forceinline__ float sign_of(float d) { return (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f); }

__global__ __launch_bounds__(FL_NT) void flow_loss_forward_kernel(FlowLossArgs a) {
  __shared__ float s_red[FL_NT / 64];
  const size_t HW = (size_t)a.H * a.W;
  const float f1 = a.fid1_dev ? a.fid1_dev[0] : a.fid1, f2 = a.fid2_dev ? a.fid2_dev[0] : a.fid2;
  const float pair = fminf(fmaxf(cosf(fabsf(f1 - f2) * FL_HALF_PI), 0.2f), 1.0f);  // train_gui.py:1105
  const float fw = (float)a.W, fh = (float)a.H, inv_c = 1.0f / (float)a.C;
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < FL_PX; j++) {
    const size_t i = (size_t)blockIdx.x * (FL_NT * FL_PX) + threadIdx.x + FL_NT * j;
    if (i < HW) {
      const bool live = (a.alpha[i] > 0.9f) && ((a.masks[i * a.MC] > 0.f) || (a.masks[i * a.MC + 1] > 0.f));
      float ad = 0.f;
      for (int c = 0; c < a.C; c++) ad += fabsf(a.image[c * HW + i] - a.gt[c * HW + i]);
      const float l1w = cosf((ad * inv_c) * FL_HALF_PI);     // :1116-1117
      const float w = ((live ? 1.0f : 0.0f) * pair) * l1w;   // :1114, :1118
      a.weight[i] = w;
      const float2 f = reinterpret_cast<const float2*>(a.flow)[i];  // (8-byte aligned: checked by the entry)
      const float cx = f.x / fw * 2.0f, cy = f.y / fh * 2.0f;  // :1101
      sum += fabsf(w * cx - w * a.motion[i]) + fabsf(w * cy - w * a.motion[HW + i]);    // :1120
    }
  }
  const float ws = wave_sum(sum);
  if ((threadIdx.x & 63) == 63) s_red[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) a.partial[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// fixed-order sum of the per-workgroup partials (deterministic), / (2 H W)
__global__ __launch_bounds__(1024) void flow_loss_finish_kernel(int n_blocks, const float* __restrict__ partial, double inv_n,
                                                                float* __restrict__ loss) {
  __shared__ double s_w[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_blocks; i += 1024) s += (double)partial[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; w++) t += s_w[w];
    loss[0] = (float)(t * inv_n);
  }
}

__global__ __launch_bounds__(FL_NT) void flow_loss_backward_kernel(FlowLossArgs a) {
  const size_t HW = (size_t)a.H * a.W;
  const float fw = (float)a.W, fh = (float)a.H;
  const float scale = a.g_loss[0] / (2.0f * (float)HW);
#pragma unroll
  for (int j = 0; j < FL_PX; j++) {
    const size_t i = (size_t)blockIdx.x * (FL_NT * FL_PX) + threadIdx.x + FL_NT * j;
    if (i < HW) {
      const float w = a.weight[i];
      float gx = 0.f, gy = 0.f;
      if (w != 0.f) {  // (a dead pixel: exact zeros)
        const float2 f = reinterpret_cast<const float2*>(a.flow)[i];
        const float cx = f.x / fw * 2.0f, cy = f.y / fh * 2.0f;
        gx = -sign_of(w * cx - w * a.motion[i]) * w * scale;
        gy = -sign_of(w * cy - w * a.motion[HW + i]) * w * scale;
      }
      a.g_motion[i] = gx;
      a.g_motion[HW + i] = gy;
      a.g_motion[2 * HW + i] = 0.f;
    }
  }
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_flow_colors_forward(int32_t N, const float* xyz, const float* d_xyz1, const float* d_xyz2, const float* full_proj1,
                              const float* full_proj2, const float* mask_logit, int64_t mask_logit_stride, float* colour,
                              riggs_stream stream) {
  RIGGS_REQUIRE(N >= 0, "bad number of Gaussians");
  if (N == 0) return 0;
  RIGGS_REQUIRE(xyz && full_proj1 && full_proj2 && colour, "NULL buffer");
  FlowColorArgs a;
  memset(&a, 0, sizeof(a));
  a.N = N; a.xyz = xyz; a.d1 = d_xyz1; a.d2 = d_xyz2; a.F1 = full_proj1; a.F2 = full_proj2;
  a.logit = mask_logit; a.logit_stride = mask_logit_stride; a.colour = colour;
  hipLaunchKernelGGL(flow_colors_forward_kernel, dim3((N + FC_NT - 1) / FC_NT), dim3(FC_NT), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_flow_colors_backward(int32_t N, const float* xyz, const float* d_xyz1, const float* d_xyz2, const float* full_proj1,
                               const float* full_proj2, const float* mask_logit, int64_t mask_logit_stride,
                               const float* dL_dcolour, float* dL_dd_xyz1, float* dL_dd_xyz2, float* dL_dmask_logit,
                               riggs_stream stream) {
  RIGGS_REQUIRE(N >= 0, "bad number of Gaussians");
  if (N == 0) return 0;
  RIGGS_REQUIRE(xyz && full_proj1 && full_proj2 && dL_dcolour, "NULL buffer");
  RIGGS_REQUIRE(dL_dd_xyz1 || dL_dd_xyz2 || dL_dmask_logit, "no gradient asked for");
  FlowColorArgs a;
  memset(&a, 0, sizeof(a));
  a.N = N; a.xyz = xyz; a.d1 = d_xyz1; a.d2 = d_xyz2; a.F1 = full_proj1; a.F2 = full_proj2;
  a.logit = mask_logit; a.logit_stride = mask_logit_stride; a.g_colour = dL_dcolour;
  a.g_d1 = dL_dd_xyz1; a.g_d2 = dL_dd_xyz2; a.g_logit = dL_dmask_logit;
  hipLaunchKernelGGL(flow_colors_backward_kernel, dim3((N + FC_NT - 1) / FC_NT), dim3(FC_NT), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

static size_t fl_blocks(int H, int W) { return ((size_t)H * W + FL_NT * FL_PX - 1) / (FL_NT * FL_PX); }

size_t riggs_flow_loss_state_floats(int32_t H, int32_t W) {
  if (H < 1 || W < 1) return 0;
  return (size_t)H * W + fl_blocks(H, W);
}

static int fl_args(FlowLossArgs& a, int32_t C, int32_t H, int32_t W, int32_t MC) {
  RIGGS_REQUIRE(C >= 1 && H >= 1 && W >= 1 && MC >= 2, "bad image shape");
  RIGGS_REQUIRE((size_t)H * W <= ((size_t)1 << 30), "image too large");
  memset(&a, 0, sizeof(a));
  a.C = C; a.H = H; a.W = W; a.MC = MC;
  return 0;
}

int riggs_flow_loss_forward(int32_t C, int32_t H, int32_t W, int32_t mask_channels, const float* image, const float* gt,
                            const float* motion, const float* alpha, const float* flow, const float* masks,
                            const float* fid1_dev, const float* fid2_dev, float fid1, float fid2, float* state, float* loss,
                            riggs_stream stream) {
  FlowLossArgs a;
  if (int rc = fl_args(a, C, H, W, mask_channels)) return rc;
  RIGGS_REQUIRE(image && gt && motion && alpha && flow && masks && state && loss, "NULL buffer");
  RIGGS_REQUIRE(((uintptr_t)flow & 7) == 0, "flow must be 8-byte aligned (it is read as pairs)");
  a.image = image; a.gt = gt; a.motion = motion; a.alpha = alpha; a.flow = flow; a.masks = masks;
  a.fid1_dev = fid1_dev; a.fid2_dev = fid2_dev; a.fid1 = fid1; a.fid2 = fid2;
  a.weight = state; a.partial = state + (size_t)H * W; a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)fl_blocks(H, W);
  hipLaunchKernelGGL(flow_loss_forward_kernel, dim3(nb), dim3(FL_NT), 0, s, a);
  hipLaunchKernelGGL(flow_loss_finish_kernel, dim3(1), dim3(1024), 0, s, nb, a.partial, 1.0 / (2.0 * (double)H * W), loss);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_flow_loss_backward(int32_t H, int32_t W, const float* motion, const float* flow, const float* state,
                             const float* g_loss, float* dL_dmotion, riggs_stream stream) {
  FlowLossArgs a;
  if (int rc = fl_args(a, 1, H, W, 2)) return rc;
  RIGGS_REQUIRE(motion && flow && state && g_loss && dL_dmotion, "NULL buffer");
  RIGGS_REQUIRE(((uintptr_t)flow & 7) == 0, "flow must be 8-byte aligned (it is read as pairs)");
  a.motion = motion; a.flow = flow; a.weight = const_cast<float*>(state); a.g_loss = g_loss; a.g_motion = dL_dmotion;
  hipLaunchKernelGGL(flow_loss_backward_kernel, dim3((int)fl_blocks(H, W)), dim3(FL_NT), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
