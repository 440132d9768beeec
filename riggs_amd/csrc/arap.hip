// ARAP handle editing of control nodes (the reference's utils/arap_deform.py: ARAPDeformer.deform, driven by lap_deform.py's
// LapDeform.deform_arap): "these M nodes go there" -> positions and rotations of all N nodes.  include/riggs_hip.h states the
// method step by step; tests/arap_ref.py restates it in NumPy.
//
// The reference solves every linear step with a dense lstsq on the N x (N - M) matrix A_u and fits the rotations with three
// batched SVDs between torch.unique / torch.nonzero read-backs.  Here the solve is ONE dense operator G = pinv(A_u) (built per
// handle set by the caller, zero rows for the handles) applied in displacement form, x = x_init + G (b - A x_init), and the whole
// drag - the initial solve and every iteration - is one launch of one workgroup per drag:
//   * rest positions, x_init, the current positions, the rotations and the right-hand side lie in LDS (21 floats per node: 84 KB
//     at N = 1024, above the 64 KB a kernel gets without asking: the entry point raises the limit once per device);
//   * a thread owns the nodes tid, tid + 512, ... and reads its own rows of the neighbour lists and weights from memory;
//   * the mat-vec streams G row by row: a wave takes four rows at a time, a lane the columns 4 lane + 256 c of each with one
//     16-byte load per c, against ITS slice of the three right-hand-side columns held in registers (read once per mat-vec from
//     the column-major LDS image, one conflict-free 16-byte LDS read per c and column); the 64 partial sums per row and column
//     meet in wave_sum's fixed DPP tree.  No float atomics, no order that depends on the batch: the same drag gives the same
//     bits alone, in any row of a batch, and on every run.
#include "common.h"
#include "fk_device.h"
#include "horn_rotation.h"

namespace riggs {

#define AE_THREADS 512
#define AE_WAVES (AE_THREADS / 64)
#define AE_ROWS 4  // rows of G in flight per wave

struct ArapEditArgs {
  int N, K, M, ld, iterations;
  const float* verts;      // (N, 3) rest positions
  const int* nn;           // (N, K), outside [0, N) = dropped
  const float* weight;     // (N, K), 0 on a dropped edge
  const float* op;         // (N, ld) G, row-major
  const int* handle_idx;   // (M)
  const float* handle_pos; // (B, M, 3)
  const float* init_verts; // (B, N, 3) or null
  float* pos_out;          // (B, N, 3)
  float* quat_out;         // (B, N, 4) or null
};

__device__ __forceinline__ int ae_nb(const ArapEditArgs& a, int i, int k) {
  const int j = a.nn[(size_t)i * a.K + k];
  return (unsigned)j < (unsigned)a.N ? j : -1;
}

// s_cur = x_init + G r, r column-major in s_r (three columns of C * 256 floats, zero beyond N).
template <int C>
__device__ __forceinline__ void ae_apply(const ArapEditArgs& a, const float* s_r, const float* s_xi, float* s_cur) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 rv[C][3];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int d = 0; d < 3; ++d) rv[c][d] = *reinterpret_cast<const float4*>(s_r + d * (C * 256) + c * 256 + 4 * lane);
  for (int row0 = wave * AE_ROWS; row0 < a.N; row0 += AE_WAVES * AE_ROWS) {  // (wave-uniform)
    float4 g[AE_ROWS][C];
#pragma unroll
    for (int r = 0; r < AE_ROWS; ++r)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int col = c * 256 + 4 * lane;
        g[r][c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < a.N && col < a.ld) g[r][c] = *reinterpret_cast<const float4*>(a.op + (size_t)(row0 + r) * a.ld + col);
      }
#pragma unroll
    for (int r = 0; r < AE_ROWS; ++r) {
      float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          acc[d] += g[r][c].x * rv[c][d].x;
          acc[d] += g[r][c].y * rv[c][d].y;
          acc[d] += g[r][c].z * rv[c][d].z;
          acc[d] += g[r][c].w * rv[c][d].w;
        }
#pragma unroll
      for (int d = 0; d < 3; ++d) acc[d] = wave_sum(acc[d]);
      const int row = row0 + r;
      if (lane == 63 && row < a.N) {
#pragma unroll
        for (int d = 0; d < 3; ++d) s_cur[3 * row + d] = s_xi[3 * row + d] + acc[d];
      }
    }
  }
}

template <int C>
__global__ void __launch_bounds__(AE_THREADS) arap_edit_kernel(ArapEditArgs a) {
  extern __shared__ __align__(16) float ae_lds[];
  const int N = a.N, K = a.K, tid = threadIdx.x, b = blockIdx.x;
  float* s_r = ae_lds;                 // 3 x (C * 256), column-major
  float* s_p0 = s_r + 3 * C * 256;     // (N, 3)
  float* s_xi = s_p0 + 3 * N;          // (N, 3) the rest positions with the handles moved
  float* s_cur = s_xi + 3 * N;         // (N, 3)
  float* s_R = s_cur + 3 * N;          // (N, 9)
  const float* hp = a.handle_pos + (size_t)b * a.M * 3;

  for (int e = tid; e < 3 * C * 256; e += AE_THREADS) s_r[e] = 0.f;
  for (int e = tid; e < 3 * N; e += AE_THREADS) { const float v = a.verts[e]; s_p0[e] = v; s_xi[e] = v; }
  for (int e = tid; e < 9 * N; e += AE_THREADS) s_R[e] = (e % 9) % 4 == 0 ? 1.f : 0.f;
  __syncthreads();
  for (int m = tid; m < a.M; m += AE_THREADS) {
    const int h = a.handle_idx[m];
    if ((unsigned)h < (unsigned)N) {
#pragma unroll
      for (int d = 0; d < 3; ++d) s_xi[3 * h + d] = hp[3 * m + d];
    }
  }
  __syncthreads();

  if (a.init_verts) {
    const float* iv = a.init_verts + (size_t)b * N * 3;
    for (int e = tid; e < 3 * N; e += AE_THREADS) s_cur[e] = iv[e];
  } else {
    // the initial solve: b = A p0, so b - A x_init = A d with d = p0 - x_init, which is zero off the handles
    for (int i = tid; i < N; i += AE_THREADS) {
      float r[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) r[d] = s_p0[3 * i + d] - s_xi[3 * i + d];
      for (int k = 0; k < K; ++k) {
        const int j = ae_nb(a, i, k);
        if (j < 0) continue;
        const float w = a.weight[(size_t)i * K + k];
#pragma unroll
        for (int d = 0; d < 3; ++d) r[d] -= w * (s_p0[3 * j + d] - s_xi[3 * j + d]);
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) s_r[d * (C * 256) + i] = r[d];
    }
    __syncthreads();
    ae_apply<C>(a, s_r, s_xi, s_cur);
  }
  __syncthreads();

  for (int it = 0; it < a.iterations; ++it) {
    // 1-2: the weighted covariance of rest edges and current edges, the reference's "unchanged" rule, the rotation
    for (int i = tid; i < N; i += AE_THREADS) {
      double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      bool same[3] = {true, true, true};
      for (int k = 0; k < K; ++k) {
        const int j = ae_nb(a, i, k);
        if (j < 0) continue;  // a padded edge is 0 at rest and now: equal on every axis
        const float w = a.weight[(size_t)i * K + k];
        float P[3], Q[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          P[d] = s_p0[3 * i + d] - s_p0[3 * j + d];
          Q[d] = s_cur[3 * i + d] - s_cur[3 * j + d];
          same[d] = same[d] && (P[d] == Q[d]);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) S[3 * r + c] += (double)w * ((double)P[r] * (double)Q[c]);
      }
      double Rd[9];
      if (same[0] || same[1] || same[2]) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Rd[e] = (e % 4 == 0) ? 1.0 : 0.0;
      } else {
        nr_horn_rotation(S, Rd);
      }
#pragma unroll
      for (int e = 0; e < 9; ++e) s_R[9 * i + e] = (float)Rd[e];
    }
    __syncthreads();
    // 3-4: b_i = 1/2 sum_k w_ik (R_i + R_j) P_ik, then b - A x_init
    for (int i = tid; i < N; i += AE_THREADS) {
      float bs[3] = {0.f, 0.f, 0.f}, ax[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) ax[d] = s_xi[3 * i + d];
      for (int k = 0; k < K; ++k) {
        const int j = ae_nb(a, i, k);
        if (j < 0) continue;
        const float w = a.weight[(size_t)i * K + k];
        float P[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) P[d] = s_p0[3 * i + d] - s_p0[3 * j + d];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          float v = 0.f;
#pragma unroll
          for (int c = 0; c < 3; ++c) v += (s_R[9 * i + 3 * r + c] + s_R[9 * j + 3 * r + c]) * P[c];
          bs[r] += w * v;
          ax[r] -= w * s_xi[3 * j + r];
        }
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) s_r[d * (C * 256) + i] = 0.5f * bs[d] - ax[d];
    }
    __syncthreads();
    // 4-5: x = x_init + G (b - A x_init); a handle's row of G is zero, so it stays on its target
    ae_apply<C>(a, s_r, s_xi, s_cur);
    __syncthreads();
  }

  float* po = a.pos_out + (size_t)b * N * 3;
  for (int e = tid; e < 3 * N; e += AE_THREADS) po[e] = s_cur[e];
  if (a.quat_out) {
    float* qo = a.quat_out + (size_t)b * N * 4;
    for (int i = tid; i < N; i += AE_THREADS) {
      float m[12], q[4];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[4 * r + c] = s_R[9 * i + 3 * r + c];
        m[4 * r + 3] = 0.f;
      }
      R_to_quat(m, q);
#pragma unroll
      for (int d = 0; d < 4; ++d) qo[4 * i + d] = q[d];
    }
  }
}

static size_t ae_lds_bytes(int N, int C) { return ((size_t)3 * C * 256 + (size_t)18 * N) * sizeof(float); }

template <int C>
static int ae_launch(const ArapEditArgs& a, int B, hipStream_t s) {
  static unsigned long long attr = 0ull;  // (per device)
  if (once_per_device(attr))
    RIGGS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(arap_edit_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)ae_lds_bytes(C * 256, C)));
  hipLaunchKernelGGL(arap_edit_kernel<C>, dim3(B), dim3(AE_THREADS), ae_lds_bytes(a.N, C), s, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_arap_edit(int32_t B, int32_t N, int32_t K, int32_t M, const float* verts, const int32_t* nn_idx, const float* weight,
                    const float* op, int32_t op_ld, const int32_t* handle_idx, const float* handle_pos, const float* init_verts,
                    int32_t iterations, float* pos_out, float* quat_out, riggs_stream stream) {
  RIGGS_REQUIRE(B >= 1 && B <= 65535, "riggs_arap_edit: 1 <= B <= 65535");
  RIGGS_REQUIRE(N >= 2 && N <= RIGGS_ARAP_EDIT_MAX_NODES, "riggs_arap_edit: 2 <= N <= 1024");
  RIGGS_REQUIRE(K >= 1 && K <= RIGGS_ARAP_EDIT_MAX_K, "riggs_arap_edit: 1 <= K <= 16");
  RIGGS_REQUIRE(M >= 1 && M <= N, "riggs_arap_edit: 1 <= M <= N handles");
  RIGGS_REQUIRE(iterations >= 0 && iterations <= 64, "riggs_arap_edit: 0 <= iterations <= 64");
  RIGGS_REQUIRE(op_ld >= N && op_ld % 4 == 0 && op_ld <= RIGGS_ARAP_EDIT_MAX_NODES, "riggs_arap_edit: op_ld is a multiple of 4, N <= op_ld <= 1024");
  RIGGS_REQUIRE(verts && nn_idx && weight && op && handle_idx && handle_pos && pos_out, "riggs_arap_edit: null pointer");
  RIGGS_REQUIRE(((uintptr_t)op & 15) == 0, "riggs_arap_edit: op must be 16-byte aligned");
  ArapEditArgs a{N, K, M, op_ld, iterations, verts, nn_idx, weight, op, handle_idx, handle_pos, init_verts, pos_out, quat_out};
  hipStream_t s = (hipStream_t)stream;
  switch ((N + 255) / 256) {
    case 1: return ae_launch<1>(a, B, s);
    case 2: return ae_launch<2>(a, B, s);
    case 3: return ae_launch<3>(a, B, s);
    default: return ae_launch<4>(a, B, s);
  }
}

}  // extern "C"
