// Stage-1 node regularisers (ControlNodeWarp.arap_loss / elastic_loss / acc_loss, utils/time_utils.py:1080-1120):
//   node-graph KNN       pytorch3d.ops.knn_points restated as "K smallest squared distances, ascending, ties to the lowest
//                        index", with cal_connectivity_from_points' slice of column 0 and radius rule (utils/deform_utils.py:51-103)
//   ARAP energy          cal_arap_error / estimate_rotation (utils/deform_utils.py:123-198), weight = None (binary edges)
//   elastic, acceleration                                  (utils/time_utils.py:1091-1120)
// The reference runs a KNN extension, boolean-mask compaction, torch.unique / torch.nonzero (host syncs), a batched 3x3 SVD and
// a few dozen small launches per call.  Here the neighbour lists stay padded (M, K) with -1 for dropped edges, the 3x3 rotation
// is Horn's quaternion form of the same Kabsch problem (a 4x4 Jacobi eigen-solve in fp64 registers), and every backward is
// deterministic without float atomics: an edge pass writes each edge's per-time gradient block, and one wave per node sums the
// blocks of the edges that touch it in a fixed lane / fixed tree order.  Scalar losses are fp64 partial sums reduced by one
// workgroup in a fixed order.
#include "common.h"
#include "horn_rotation.h"

namespace riggs {

#define NR_KMAX 16   // K + 1 <= 16 neighbour columns
#define NR_DMAX 16   // coordinates per point
#define NR_TMAX 16   // time samples
#define NR_MMAX 8192
#define NR_KNN_SPLIT 8                      // lanes per query, each scanning its share of every LDS tile
#define NR_KNN_TILE 256                     // points per LDS tile
#define NR_KNN_QPB (256 / NR_KNN_SPLIT)     // queries per workgroup

// ---- node-graph KNN ------------------------------------------------------------------------------------------------------
// (d, index) lexicographic insert into an ascending list of KQ entries (compile-time indices only: the list stays in VGPRs)
__device__ __forceinline__ bool nr_lt(float d, int j, float bd, int bj) { return d < bd || (d == bd && j < bj); }
template <int KQ>
__device__ __forceinline__ void nr_insert(float (&bd)[KQ], int (&bi)[KQ], float d, int j) {
  if (!nr_lt(d, j, bd[KQ - 1], bi[KQ - 1])) return;
#pragma unroll
  for (int k = KQ - 1; k >= 0; --k) {
    const int u = k > 0 ? k - 1 : 0;
    if (k > 0 && nr_lt(d, j, bd[u], bi[u])) { bd[k] = bd[u]; bi[k] = bi[u]; }
    else if (nr_lt(d, j, bd[k], bi[k])) { bd[k] = d; bi[k] = j; }
  }
}

struct KnnArgs {
  int M, D, stride, Kq, drop, least, Kout;
  float radius2;  // > 0: columns >= least (after the drop) at or beyond it become -1 / inf
  const float* pts;
  int* idx; float* dist;
};

// NR_KNN_SPLIT lanes per query: lane s scans points s, s + SPLIT, ... of every staged tile in ascending index, keeps its own
// sorted list; the lists are merged through LDS by the query's first lane with the (d, index) order.
template <int KQ>
__global__ void __launch_bounds__(256) node_knn_kernel(KnnArgs a) {
  __shared__ float s_pts[NR_KNN_TILE * NR_DMAX];
  __shared__ float s_d[256 * KQ];
  __shared__ int s_i[256 * KQ];
  const int ql = threadIdx.x / NR_KNN_SPLIT, sp = threadIdx.x % NR_KNN_SPLIT;
  const int q = blockIdx.x * NR_KNN_QPB + ql;
  const bool live = q < a.M;
  float x[NR_DMAX];
#pragma unroll
  for (int c = 0; c < NR_DMAX; ++c) x[c] = (live && c < a.D) ? a.pts[(size_t)q * a.stride + c] : 0.f;
  float bd[KQ]; int bi[KQ];
#pragma unroll
  for (int k = 0; k < KQ; ++k) { bd[k] = INFINITY; bi[k] = 0x7fffffff; }
  for (int base = 0; base < a.M; base += NR_KNN_TILE) {
    const int cnt = min(NR_KNN_TILE, a.M - base);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * a.D; e += 256) {
      const int p = e / a.D, c = e % a.D;
      s_pts[p * NR_DMAX + c] = a.pts[(size_t)(base + p) * a.stride + c];
    }
    __syncthreads();
    if (live) {
      for (int p = sp; p < cnt; p += NR_KNN_SPLIT) {
        const float* y = s_pts + p * NR_DMAX;
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < NR_DMAX; ++c)
          if (c < a.D) { const float t = x[c] - y[c]; d = d + t * t; }
        nr_insert<KQ>(bd, bi, d, base + p);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KQ; ++k) { s_d[threadIdx.x * KQ + k] = bd[k]; s_i[threadIdx.x * KQ + k] = bi[k]; }
  __syncthreads();
  if (!live || sp != 0) return;
  for (int o = 1; o < NR_KNN_SPLIT; ++o) {
    const int src = (threadIdx.x + o) * KQ;
    for (int k = 0; k < KQ; ++k) {
      if (s_i[src + k] == 0x7fffffff) break;
      nr_insert<KQ>(bd, bi, s_d[src + k], s_i[src + k]);
    }
  }
#pragma unroll
  for (int k = 0; k < KQ; ++k) {
    if (k < a.drop) continue;
    const int c = k - a.drop;
    int j = bi[k];
    float d = bd[k];
    if (j == 0x7fffffff) { j = -1; d = INFINITY; }  // fewer than Kq points
    if (a.radius2 > 0.f && c >= a.least && !(d < a.radius2)) { j = -1; d = INFINITY; }
    a.idx[(size_t)q * a.Kout + c] = j;
    a.dist[(size_t)q * a.Kout + c] = d;
  }
}

// ---- fixed-order scalar reduction: fp64 partials -> one fp32 value ---------------------------------------------------------
__global__ void __launch_bounds__(256) nr_reduce_kernel(const double* part, int n, double scale, float* out) {
  __shared__ double s[256];
  double v = 0.0;
  for (int e = threadIdx.x; e < n; e += 256) v += part[e];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(s[0] * scale);
}

// ---- deterministic per-node gather of edge gradient blocks ---------------------------------------------------------------
// out[m] = sum over edges e with plus[e] == m of G[e] - sum over edges with minus[e] == m of G[e]; G[e] is T x 3 floats.
// One wave per node; lane l takes edges l, l + 64, ... in ascending order, then a fixed DPP tree over the lanes.
// out index: m * om + t * ot + c.
__global__ void __launch_bounds__(256) nr_gather_kernel(int M, int E, int T, const int* plus, const int* minus, const float* G,
                                                        float* out, int om, int ot) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= M) return;  // (wave-uniform)
  float acc[NR_TMAX * 3];
#pragma unroll
  for (int w = 0; w < NR_TMAX * 3; ++w) acc[w] = 0.f;
  const int W = T * 3;
  for (int e = lane; e < E; e += 64) {
    const float sg = (plus[e] == m ? 1.f : 0.f) - (minus[e] == m ? 1.f : 0.f);
    if (plus[e] == m || minus[e] == m) {
      const float* g = G + (size_t)e * W;
#pragma unroll
      for (int w = 0; w < NR_TMAX * 3; ++w)
        if (w < W) acc[w] += sg * g[w];
    }
  }
#pragma unroll
  for (int w = 0; w < NR_TMAX * 3; ++w) {
    if (w < W) {
      const float v = wave_sum(acc[w]);
      if (lane == 63) out[(size_t)m * om + (size_t)(w / 3) * ot + (w % 3)] = v;
    }
  }
}

// ---- ARAP ----------------------------------------------------------------------------------------------------------------
// (the rotation fit itself, nr_horn_rotation, is horn_rotation.h: arap.hip fits with the same code)
struct ArapArgs {
  int M, T, K, Ns;
  const float* seq;  // (T, M, 3)
  const int* nn;     // (M, K), -1 = dropped
  const int* rows;   // (Ns) sample rows
  float* rot;        // (Ns, T, 9), t = 0 unused
};

// indices outside [0, M) (sample rows or neighbours) count as dropped edges: never read, no contribution
__device__ __forceinline__ int nr_node(int j, int M) { return (unsigned)j < (unsigned)M ? j : -1; }
__device__ __forceinline__ int arap_nb(const ArapArgs& a, int i, int n) {
  return (unsigned)i < (unsigned)a.M ? nr_node(a.nn[(size_t)i * a.K + n], a.M) : -1;
}

__device__ __forceinline__ void nr_edges(const ArapArgs& a, int i, int j, int t, float src[3], float tgt[3]) {
  const float* p0 = a.seq;
  const float* pt = a.seq + (size_t)t * a.M * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) { src[c] = 0.f; tgt[c] = 0.f; }
  if (j < 0) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) { src[c] = p0[3 * i + c] - p0[3 * j + c]; tgt[c] = pt[3 * i + c] - pt[3 * j + c]; }
}

// one thread per (sample row, t >= 1): S, the unchanged-vertex rule, R, and sum_n w |tgt - R src|^2
__global__ void __launch_bounds__(256) arap_forward_kernel(ArapArgs a, double* part) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.Ns * a.T) return;
  const int s = g / a.T, t = g % a.T;
  if (t == 0) { part[g] = 0.0; return; }
  const int i = a.rows[s];
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool same[3] = {true, true, true};
  for (int n = 0; n < a.K; ++n) {
    const int j = arap_nb(a, i, n);
    float src[3], tgt[3];
    nr_edges(a, i, j, t, src, tgt);
#pragma unroll
    for (int c = 0; c < 3; ++c) same[c] = same[c] && (src[c] == tgt[c]);
    if (j < 0) continue;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[3 * r + c] += (double)src[r] * (double)tgt[c];
  }
  double Rd[9];
  if (same[0] || same[1] || same[2]) {
#pragma unroll
    for (int e = 0; e < 9; ++e) Rd[e] = (e % 4 == 0) ? 1.0 : 0.0;
  } else {
    nr_horn_rotation(S, Rd);
  }
  float* Ro = a.rot + (size_t)g * 9;
  double R[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) { Ro[e] = (float)Rd[e]; R[e] = (double)(float)Rd[e]; }
  double en = 0.0;
  for (int n = 0; n < a.K; ++n) {
    const int j = arap_nb(a, i, n);
    if (j < 0) continue;
    float src[3], tgt[3];
    nr_edges(a, i, j, t, src, tgt);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double v = (double)tgt[r] - (R[3 * r] * src[0] + R[3 * r + 1] * src[1] + R[3 * r + 2] * src[2]);
      en += v * v;
    }
  }
  part[g] = en;
}

// one thread per (sample row, neighbour column): the edge's gradient block, slot t >= 1 = dE/dtgt_t, slot 0 = sum_t dE/dsrc
__global__ void __launch_bounds__(256) arap_edge_backward_kernel(ArapArgs a, const float* g_loss, int* plus, int* minus, float* G) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.Ns * a.K) return;
  const int s = e / a.K, n = e % a.K;
  const int i = a.rows[s];
  const int j = arap_nb(a, i, n);
  plus[e] = j >= 0 ? i : -1;
  minus[e] = j >= 0 ? j : -1;
  if (j < 0) return;
  const double gl = (double)g_loss[0];
  double g0[3] = {0, 0, 0};
  float* Ge = G + (size_t)e * a.T * 3;
  for (int t = 1; t < a.T; ++t) {
    float src[3], tgt[3];
    nr_edges(a, i, j, t, src, tgt);
    const float* Rf = a.rot + ((size_t)s * a.T + t) * 9;
    double R[9], r[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = (double)Rf[q];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = (double)tgt[c] - (R[3 * c] * src[0] + R[3 * c + 1] * src[1] + R[3 * c + 2] * src[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Ge[3 * t + c] = (float)(2.0 * gl * r[c]);
      g0[c] -= 2.0 * gl * (R[c] * r[0] + R[3 + c] * r[1] + R[6 + c] * r[2]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) Ge[c] = (float)g0[c];
}

// ---- elastic -------------------------------------------------------------------------------------------------------------
struct ElasticArgs {
  int M, T, K;
  const float* x;   // (M, T, 3) node positions over T samples
  const int* nn;    // (M, K), -1 = none
  const float* w;   // (M, K) weights
};

// edge lengths over T, their mean and unbiased variance (fp64 from the fp32 lengths); arrays indexed by unrolled constants only
__device__ __forceinline__ void el_stats(const ElasticArgs& a, int m, int j, float (&len)[NR_TMAX], float (&dv)[NR_TMAX][3],
                                         double& mean, double& var) {
  mean = 0.0;
#pragma unroll
  for (int t = 0; t < NR_TMAX; ++t) {
    len[t] = 0.f;
    if (t < a.T) {
      const float* pm = a.x + ((size_t)m * a.T + t) * 3;
      const float* pj = a.x + ((size_t)j * a.T + t) * 3;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) { dv[t][c] = pj[c] - pm[c]; s = s + dv[t][c] * dv[t][c]; }
      len[t] = sqrtf(s);
      mean += (double)len[t];
    }
  }
  mean /= a.T;
  var = 0.0;
#pragma unroll
  for (int t = 0; t < NR_TMAX; ++t)
    if (t < a.T) { const double d = (double)len[t] - mean; var += d * d; }
  var /= (a.T - 1);
}

__global__ void __launch_bounds__(256) elastic_forward_kernel(ElasticArgs a, double* part) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.M * a.K) return;
  const int m = e / a.K, j = nr_node(a.nn[e], a.M);
  if (j < 0) { part[e] = 0.0; return; }
  float len[NR_TMAX], dv[NR_TMAX][3];
  double mean, var;
  el_stats(a, m, j, len, dv, mean, var);
  part[e] = (double)a.w[e] * (var / (var + 1e-5));
}

__global__ void __launch_bounds__(256) elastic_edge_backward_kernel(ElasticArgs a, const float* g_loss, float* g_w, int* plus,
                                                                    int* minus, float* G) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.M * a.K) return;
  const int m = e / a.K, j = nr_node(a.nn[e], a.M);
  plus[e] = j >= 0 ? j : -1;
  minus[e] = j >= 0 ? m : -1;
  if (j < 0) { g_w[e] = 0.f; return; }
  float len[NR_TMAX], dv[NR_TMAX][3];
  double mean, var;
  el_stats(a, m, j, len, dv, mean, var);
  const double gl = (double)g_loss[0] / a.M;
  g_w[e] = (float)(gl * (var / (var + 1e-5)));
  const double coef = gl * (double)a.w[e] / (var + 1e-5) * 2.0 / (a.T - 1);
  float* Ge = G + (size_t)e * a.T * 3;
#pragma unroll
  for (int t = 0; t < NR_TMAX; ++t) {
    if (t < a.T) {
      const double f = len[t] > 0.f ? coef * ((double)len[t] - mean) / (double)len[t] : 0.0;  // |.|' = 0 at 0, as torch
#pragma unroll
      for (int c = 0; c < 3; ++c) Ge[3 * t + c] = (float)(f * dv[t][c]);
    }
  }
}

// ---- acceleration --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float acc_vec(const float* x, int m, float d[3]) {
  const float* p = x + (size_t)m * 9;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) { d[c] = p[c] + p[6 + c] - 2.0f * p[3 + c]; s = s + d[c] * d[c]; }
  return sqrtf(s);
}

__global__ void __launch_bounds__(256) acc_forward_kernel(int M, const float* x, double* part) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float d[3];
  const float n = acc_vec(x, m, d);
  part[m] = (double)n / ((double)n + 1e-5);
}

__global__ void __launch_bounds__(256) acc_backward_kernel(int M, const float* x, const float* g_loss, float* g_x) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float d[3];
  const float n = acc_vec(x, m, d);
  const double f = n > 0.f ? (double)g_loss[0] / M / ((double)n + 1e-5) / (double)n : 0.0;
  float* g = g_x + (size_t)m * 9;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float u = (float)(f * d[c]);
    g[c] = u; g[3 + c] = -2.0f * u; g[6 + c] = u;
  }
}

// ---- workspace layouts (bytes, 256-aligned) ------------------------------------------------------------------------------
struct EdgeWs { size_t part, plus, minus, G, total; };
static EdgeWs edge_ws(size_t nparts, size_t E, int T) {
  EdgeWs w;
  size_t o = 0;
  w.part = o; o += align_up(nparts * sizeof(double));
  w.plus = o; o += align_up(E * sizeof(int));
  w.minus = o; o += align_up(E * sizeof(int));
  w.G = o; o += align_up(E * (size_t)T * 3 * sizeof(float));
  w.total = o;
  return w;
}

static inline unsigned nblk(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_node_knn(int32_t M, int32_t D, int32_t stride, int32_t Kq, int32_t drop_first, int32_t least_edge_num, float radius2,
                   const float* points, int32_t* nn_idx, float* nn_dist, riggs_stream stream) {
  RIGGS_REQUIRE(M >= 1 && M <= NR_MMAX, "riggs_node_knn: 1 <= M <= 8192");
  RIGGS_REQUIRE(D >= 1 && D <= NR_DMAX && stride >= D, "riggs_node_knn: 1 <= D <= 16, stride >= D");
  RIGGS_REQUIRE(Kq >= 1 && Kq <= NR_KMAX, "riggs_node_knn: 1 <= K + 1 <= 16");
  RIGGS_REQUIRE(drop_first == 0 || drop_first == 1, "riggs_node_knn: drop_first is 0 or 1");
  RIGGS_REQUIRE(Kq - drop_first >= 1, "riggs_node_knn: no column left");
  RIGGS_REQUIRE(points && nn_idx && nn_dist, "riggs_node_knn: null pointer");
  hipStream_t s = (hipStream_t)stream;
  KnnArgs a{M, D, stride, Kq, drop_first, least_edge_num, Kq - drop_first, radius2, points, nn_idx, nn_dist};
  const dim3 grid(nblk(M, NR_KNN_QPB));
  switch (Kq) {
#define NR_KNN_CASE(KQ) case KQ: hipLaunchKernelGGL(node_knn_kernel<KQ>, grid, dim3(256), 0, s, a); break;
    NR_KNN_CASE(1) NR_KNN_CASE(2) NR_KNN_CASE(3) NR_KNN_CASE(4) NR_KNN_CASE(5) NR_KNN_CASE(6) NR_KNN_CASE(7) NR_KNN_CASE(8)
    NR_KNN_CASE(9) NR_KNN_CASE(10) NR_KNN_CASE(11) NR_KNN_CASE(12) NR_KNN_CASE(13) NR_KNN_CASE(14) NR_KNN_CASE(15) NR_KNN_CASE(16)
#undef NR_KNN_CASE
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

static int arap_check(int32_t M, int32_t T, int32_t K, int32_t Ns) {
  RIGGS_REQUIRE(M >= 1 && M <= NR_MMAX, "riggs_arap: 1 <= M <= 8192");
  RIGGS_REQUIRE(T >= 1 && T <= NR_TMAX, "riggs_arap: 1 <= T <= 16");
  RIGGS_REQUIRE(K >= 1 && K <= NR_KMAX - 1, "riggs_arap: 1 <= K <= 15");
  RIGGS_REQUIRE(Ns >= 1 && Ns <= NR_MMAX, "riggs_arap: 1 <= sample rows <= 8192");
  return 0;
}

size_t riggs_arap_workspace_floats(int32_t M, int32_t T, int32_t K, int32_t Ns) {
  (void)M;
  return edge_ws((size_t)Ns * T, (size_t)Ns * K, T).total / sizeof(float);
}

int riggs_arap_forward(int32_t M, int32_t T, int32_t K, int32_t Ns, const float* seq, const int32_t* nn_idx, const int32_t* rows,
                       float* rot, float* loss, float* workspace, riggs_stream stream) {
  if (int rc = arap_check(M, T, K, Ns)) return rc;
  RIGGS_REQUIRE(seq && nn_idx && rows && rot && loss && workspace, "riggs_arap_forward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const EdgeWs w = edge_ws((size_t)Ns * T, (size_t)Ns * K, T);
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + w.part);
  ArapArgs a{M, T, K, Ns, seq, nn_idx, rows, rot};
  hipLaunchKernelGGL(arap_forward_kernel, dim3(nblk((size_t)Ns * T, 256)), dim3(256), 0, s, a, part);
  hipLaunchKernelGGL(nr_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)part, Ns * T, 1.0, loss);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_arap_backward(int32_t M, int32_t T, int32_t K, int32_t Ns, const float* seq, const int32_t* nn_idx, const int32_t* rows,
                        const float* rot, const float* g_loss, float* g_seq, float* workspace, riggs_stream stream) {
  if (int rc = arap_check(M, T, K, Ns)) return rc;
  RIGGS_REQUIRE(seq && nn_idx && rows && rot && g_loss && g_seq && workspace, "riggs_arap_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const EdgeWs w = edge_ws((size_t)Ns * T, (size_t)Ns * K, T);
  char* ws = reinterpret_cast<char*>(workspace);
  int* plus = reinterpret_cast<int*>(ws + w.plus);
  int* minus = reinterpret_cast<int*>(ws + w.minus);
  float* G = reinterpret_cast<float*>(ws + w.G);
  ArapArgs a{M, T, K, Ns, seq, nn_idx, rows, const_cast<float*>(rot)};
  const int E = Ns * K;
  hipLaunchKernelGGL(arap_edge_backward_kernel, dim3(nblk(E, 256)), dim3(256), 0, s, a, g_loss, plus, minus, G);
  hipLaunchKernelGGL(nr_gather_kernel, dim3(nblk(M, 4)), dim3(256), 0, s, M, E, T, (const int*)plus, (const int*)minus,
                     (const float*)G, g_seq, 3, M * 3);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

static int elastic_check(int32_t M, int32_t T, int32_t K) {
  RIGGS_REQUIRE(M >= 1 && M <= NR_MMAX, "riggs_elastic: 1 <= M <= 8192");
  RIGGS_REQUIRE(T >= 2 && T <= NR_TMAX, "riggs_elastic: 2 <= T <= 16 (unbiased variance)");
  RIGGS_REQUIRE(K >= 1 && K <= NR_KMAX - 1, "riggs_elastic: 1 <= K <= 15");
  return 0;
}

size_t riggs_elastic_workspace_floats(int32_t M, int32_t T, int32_t K) {
  return edge_ws((size_t)M * K, (size_t)M * K, T).total / sizeof(float);
}

int riggs_elastic_forward(int32_t M, int32_t T, int32_t K, const float* nodes_t, const int32_t* nn_idx, const float* weight,
                          float* loss, float* workspace, riggs_stream stream) {
  if (int rc = elastic_check(M, T, K)) return rc;
  RIGGS_REQUIRE(nodes_t && nn_idx && weight && loss && workspace, "riggs_elastic_forward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const EdgeWs w = edge_ws((size_t)M * K, (size_t)M * K, T);
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + w.part);
  ElasticArgs a{M, T, K, nodes_t, nn_idx, weight};
  hipLaunchKernelGGL(elastic_forward_kernel, dim3(nblk((size_t)M * K, 256)), dim3(256), 0, s, a, part);
  hipLaunchKernelGGL(nr_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)part, M * K, 1.0 / M, loss);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_elastic_backward(int32_t M, int32_t T, int32_t K, const float* nodes_t, const int32_t* nn_idx, const float* weight,
                           const float* g_loss, float* g_nodes_t, float* g_weight, float* workspace, riggs_stream stream) {
  if (int rc = elastic_check(M, T, K)) return rc;
  RIGGS_REQUIRE(nodes_t && nn_idx && weight && g_loss && g_nodes_t && g_weight && workspace, "riggs_elastic_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const EdgeWs w = edge_ws((size_t)M * K, (size_t)M * K, T);
  char* ws = reinterpret_cast<char*>(workspace);
  int* plus = reinterpret_cast<int*>(ws + w.plus);
  int* minus = reinterpret_cast<int*>(ws + w.minus);
  float* G = reinterpret_cast<float*>(ws + w.G);
  ElasticArgs a{M, T, K, nodes_t, nn_idx, weight};
  const int E = M * K;
  hipLaunchKernelGGL(elastic_edge_backward_kernel, dim3(nblk(E, 256)), dim3(256), 0, s, a, g_loss, g_weight, plus, minus, G);
  hipLaunchKernelGGL(nr_gather_kernel, dim3(nblk(M, 4)), dim3(256), 0, s, M, E, T, (const int*)plus, (const int*)minus,
                     (const float*)G, g_nodes_t, T * 3, 3);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

size_t riggs_acc_workspace_floats(int32_t M) { return align_up((size_t)M * sizeof(double)) / sizeof(float); }

int riggs_acc_forward(int32_t M, const float* nodes_t, float* loss, float* workspace, riggs_stream stream) {
  RIGGS_REQUIRE(M >= 1 && M <= NR_MMAX, "riggs_acc: 1 <= M <= 8192");
  RIGGS_REQUIRE(nodes_t && loss && workspace, "riggs_acc_forward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(acc_forward_kernel, dim3(nblk(M, 256)), dim3(256), 0, s, M, nodes_t, part);
  hipLaunchKernelGGL(nr_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)part, M, 1.0 / M, loss);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_acc_backward(int32_t M, const float* nodes_t, const float* g_loss, float* g_nodes_t, riggs_stream stream) {
  RIGGS_REQUIRE(M >= 1 && M <= NR_MMAX, "riggs_acc: 1 <= M <= 8192");
  RIGGS_REQUIRE(nodes_t && g_loss && g_nodes_t, "riggs_acc_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(acc_backward_kernel, dim3(nblk(M, 256)), dim3(256), 0, s, M, nodes_t, g_loss, g_nodes_t);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
