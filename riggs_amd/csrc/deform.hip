// Skeleton-driven deformation of the Gaussian cloud:
//   fk_*   : forward kinematics over <= 64 joints on ONE wave64, <= 256 on one workgroup (replaces ~3*J torch
//            launches of SkeletonWarp.chain_product_transform, skeleton_warp.py:242-273)
//   lbs_*  : bone-distance skinning weights + linear blend skinning fused per Gaussian, with the
//            <= 63 (<= 255: the MAX_J_WIDE instantiations) bone records (segment, radius, 3x4 transform, quaternion) staged in LDS.
// The skinning forward is ONE template over the joint capacity (MAX_J / MAX_J_WIDE) and the form of the top-K selection set
// (SelReg / SelLds), with one topk_select and one topk_emit_ascending.  Where the same lines still stand in several kernels (the
// chain's write-out in its four kernels, the accumulate step and the write-out of the LDS and the scalar forward, the walk of the
// two bone-lane backwards, the top-K backward on either side of 64 joints) a shared form changed the compiler's output for a
// kernel on the benchmark's path, or measured slower: NOTES.md "deform: one body per step".
// Backward reduces over the N Gaussians inside the kernel: wave64 DPP sums -> LDS -> one atomic
// per workgroup per output.
//   playback (inference only, at the end of the file): fk_sequence_* / lbs_sequence_kernel skin a whole pose track over one cloud,
//            skinning_colors_kernel folds the same weights into a colour per Gaussian.  Shared with the forward: Bone, bone_geometry,
//            bone_d2 / bone_d2_fast, topk_select, fast_exp and the chain; restated for these kernels only: the chain's write-out,
//            the weight_mod tile, the line that forms v_k (fk_write_out, stage_mod_tile, bone_weight).
#include <type_traits>

#include "fk_device.h"

namespace riggs {

__global__ __launch_bounds__(64) void fk_forward_kernel(int J, const float* __restrict__ local_rot,
                                                        const float* __restrict__ joints,
                                                        const int32_t* __restrict__ parents,
                                                        const float* __restrict__ global_trans,
                                                        float* __restrict__ transforms, float* __restrict__ node_rot,
                                                        float* __restrict__ d_nodes) {
  FkIn in;
  fk_load(J, local_rot, joints, parents, nullptr, nullptr, in);
  FkLane f;
  fk_wave_forward(J, in, f);
  const int j = threadIdx.x;
  if (j < J) {
    const float x = in.x[0], y = in.x[1], z = in.x[2];
#pragma unroll
    for (int e = 0; e < 12; e++) transforms[12 * j + e] = f.G[e];
#pragma unroll
    for (int r = 0; r < 3; r++)
      d_nodes[3 * j + r] = (f.G[4 * r] * x + f.G[4 * r + 1] * y + f.G[4 * r + 2] * z + f.G[4 * r + 3]) + global_trans[r];
    float q[4];
    R_to_quat(f.G, q);
#pragma unroll
    for (int e = 0; e < 4; e++) node_rot[4 * j + e] = q[e];
  }
}

__global__ __launch_bounds__(64) void fk_backward_kernel(int J, const float* __restrict__ local_rot,
                                                         const float* __restrict__ joints,
                                                         const int32_t* __restrict__ parents,
                                                         const float* __restrict__ dL_dG_in,
                                                         const float* __restrict__ dL_dnodes,
                                                         float* __restrict__ dL_dlocal_rot,
                                                         float* __restrict__ dL_dglobal_trans) {
  FkIn in;
  fk_load(J, local_rot, joints, parents, dL_dG_in, dL_dnodes, in);
  FkLane f;
  fk_wave_forward(J, in, f);
  const int j = threadIdx.x;
  if (dL_dnodes && j < 3) {  // d_nodes = posed + global_trans
    float s = 0.f;
    for (int k = 0; k < J; k++) s += dL_dnodes[3 * k + j];
    dL_dglobal_trans[j] += s;
  }
  float dq[4];
  fk_wave_backward(J, in, f, dq);
  if (j < J) {
#pragma unroll
    for (int e = 0; e < 4; e++) dL_dlocal_rot[4 * j + e] = dq[e];
  }
}

// ------------------------------------------------------------------------------------ LBS
struct Bone {        // 24 floats, LDS resident
  float a[3];        // parent joint (segment start)  skeleton_warp.py:208-209
  float len2c;       // max(|b-a|^2, 1e-6)            :226
  float ba[3];       // b - a
  float inv2r2;      // 1 / (2 exp(rho)^2)            :65-66
  float G[12];       // global transform of the CHILD joint
  float q[4];        // node_rot of the child joint (detached)
  float rl2;         // 1 / len2c (the all-bones path: no top-K ties to reproduce, so no IEEE division per bone and Gaussian)
  float pad_[3];     // (records stay multiples of 16 bytes: whole-record ds_read_b128)
};

struct LbsArgs {
  int N, J, K;
  const float *x, *joints, *node_radius_log, *transforms, *node_rot, *global_trans, *motion_mask;
  const float* weight_mod;  // (N, J-1) or NULL: sigmoid(WeightMLP(x)) multiplying the kernel weights (skeleton_warp.py:56-69)
  float* dmod;              // backward: dL/dweight_mod (N, J-1) or NULL
  const int32_t* parents;
  float *d_xyz, *d_rot, *nn_weight;
  int64_t* nn_idx;
  // backward
  const float *g_xyz, *g_rot;
  float *dG, *drho, *dgt, *dmask;
  float* partial;  // [workgroups][(J-1)*13 + 3] per-workgroup sums (two-stage reduction; the second stage runs in a fixed order)
  // forward with the kinematic chain inside (riggs_lbs_forward_fk): the pose, and where workgroup 0 leaves the chain's results
  const float* local_rot;
  float *fk_transforms, *fk_node_rot, *fk_d_nodes;
  int mod_lds;  // forward: weight_mod is staged through LDS (the launch reserved the tile)
  // the caller's bone table (<= 64 joints; struct Bone below): the forward's workgroup 0 leaves its staged records there, the
  // backward stages from them — one coalesced read instead of building every record again in every workgroup
  Bone* table_out;
  const Bone* table_in;
};

// (transforms / node_rot: global memory, or the LDS arrays of a kinematic chain that this workgroup ran itself)
__device__ __forceinline__ void stage_bones(const LbsArgs& a, Bone* bones, const float* transforms, const float* node_rot);
// (the backward, given the forward's table: the records as the forward staged them — bone_geometry's two dependent loads, exp and
// divisions, and the gather of G and q, are not repeated; sizeof(Bone) is a multiple of 16)
__device__ __forceinline__ void stage_bones(const LbsArgs& a, Bone* bones) {
  if (a.table_in) {
    const float4* src = reinterpret_cast<const float4*>(a.table_in);
    float4* dst = reinterpret_cast<float4*>(bones);
    for (int e = threadIdx.x; e < (a.J - 1) * (int)(sizeof(Bone) / 16); e += blockDim.x) dst[e] = src[e];
    __syncthreads();
    return;
  }
  stage_bones(a, bones, a.transforms, a.node_rot);
}
// the part of bone k's record that no pose changes: the segment, its clamped squared length, 1 / (2 r^2)
__device__ __forceinline__ void bone_geometry(const LbsArgs& a, int k, Bone& b) {
  const int child = k + 1, par = a.parents[child];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    b.a[c] = a.joints[3 * par + c];
    b.ba[c] = a.joints[3 * child + c] - b.a[c];
  }
  const float l2 = __fadd_rn(__fadd_rn(__fmul_rn(b.ba[0], b.ba[0]), __fmul_rn(b.ba[1], b.ba[1])), __fmul_rn(b.ba[2], b.ba[2]));
  b.len2c = fmaxf(l2, 1e-6f);
  b.rl2 = 1.0f / b.len2c;
  b.pad_[0] = 0.f; b.pad_[1] = 0.f; b.pad_[2] = 0.f;
  const float rad = expf(a.node_radius_log[child]);
  b.inv2r2 = 1.0f / (2.0f * rad * rad);
}
__device__ __forceinline__ void stage_bones(const LbsArgs& a, Bone* bones, const float* transforms, const float* node_rot) {
  for (int k = threadIdx.x; k < a.J - 1; k += blockDim.x) {
    const int child = k + 1;
    Bone b;
    bone_geometry(a, k, b);
#pragma unroll
    for (int e = 0; e < 12; e++) b.G[e] = transforms[12 * child + e];
#pragma unroll
    for (int e = 0; e < 4; e++) b.q[e] = node_rot[4 * child + e];
    bones[k] = b;
  }
  __syncthreads();
}

// line_segment_distance (skeleton_warp.py:215-238), squared.  Written in the reference's own
// operation order with FP contraction off: bones that share a joint give near-tied distances
// and the top-K selection (K > 0) must break those ties the way the reference's arithmetic does.
__device__ __forceinline__ float bone_d2(const Bone& b, float px, float py, float pz) {
#pragma clang fp contract(off)
  const float ex = px - b.a[0], ey = py - b.a[1], ez = pz - b.a[2];
  float t = ((ex * b.ba[0] + ey * b.ba[1]) + ez * b.ba[2]) / b.len2c;
  t = fminf(fmaxf(t, 0.0f), 1.0f);
  const float sx = (b.a[0] + t * b.ba[0]) - px, sy = (b.a[1] + t * b.ba[1]) - py, sz = (b.a[2] + t * b.ba[2]) - pz;
  return (sx * sx + sy * sy) + sz * sz;
}

// The same distance for the all-bones configuration (K = -1): nothing is selected by comparing distances there, so the
// division becomes a multiplication by the staged reciprocal and contraction is allowed (an IEEE division is ~10 of this
// function's ~30 instructions, and it runs once per bone and Gaussian).
__device__ __forceinline__ float bone_d2_fast(const Bone& b, float px, float py, float pz) {
  const float ex = px - b.a[0], ey = py - b.a[1], ez = pz - b.a[2];
  const float t = __builtin_amdgcn_fmed3f((ex * b.ba[0] + ey * b.ba[1] + ez * b.ba[2]) * b.rl2, 0.0f, 1.0f);
  const float sx = t * b.ba[0] - ex, sy = t * b.ba[1] - ey, sz = t * b.ba[2] - ez;
  return sx * sx + sy * sy + sz * sz;
}

// The selection set of the top-K configuration (K > 0), one per thread, in two forms with one interface:
//   <= 64 joints: a 64-bit mask in registers;
//   <= 256 joints: 256 bits as a column of an LDS array (word w of thread t at col[w][t]: conflict-free).  A walk over
//   k = 0, 1, .. reloads the 32-bit word where k enters it ((k & 31) == 0): test() is for such ascending walks.
struct SelReg {
  static constexpr bool in_lds = false;
  uint64_t m;
  __device__ __forceinline__ void clear() { m = 0; }
  __device__ __forceinline__ bool test(int k) { return (m >> k) & 1ull; }
  __device__ __forceinline__ void set(int k) { m |= 1ull << k; }
  __device__ __forceinline__ void reset(int k) { m &= ~(1ull << k); }
};
struct SelLds {
  static constexpr bool in_lds = true;
  typedef uint32_t Column[FK_WIDE_WORDS][256];
  uint32_t (*col)[256];
  uint32_t w;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < FK_WIDE_WORDS; i++) col[i][threadIdx.x] = 0u;
    w = 0u;
  }
  __device__ __forceinline__ bool test(int k) {
    if ((k & 31) == 0) w = col[k >> 5][threadIdx.x];
    return (w >> (k & 31)) & 1u;
  }
  __device__ __forceinline__ void set(int k) { col[k >> 5][threadIdx.x] |= 1u << (k & 31); }
  __device__ __forceinline__ void reset(int k) { col[k >> 5][threadIdx.x] &= ~(1u << (k & 31)); }
};

// Top-K selection (K > 0): the set of the K bones with the smallest (d2, index), found by K
// selection passes over the bones.  Already-picked bones are excluded through the set, so
// no floating-point value is ever compared for equality across call sites.
template <class Sel>
__device__ __forceinline__ void topk_select(Sel& sel, const Bone* bones, int B, int K, float px, float py, float pz) {
  sel.clear();
  for (int s = 0; s < K; s++) {
    float best = INFINITY;
    int bi = -1;
    for (int k = 0; k < B; k++) {
      if (sel.test(k)) continue;
      const float d2 = bone_d2(bones[k], px, py, pz);
      if (d2 < best || bi < 0) { best = d2; bi = k; }
    }
    sel.set(bi);
  }
}
// nn_weight / nn_idx of Gaussian n in ascending-d2 order like torch.topk(largest=False): K selection passes inside the set
// (cleared as they go)
template <class Sel>
__device__ __forceinline__ void topk_emit_ascending(Sel& sel, const Bone* bones, int B, int K, float px, float py, float pz,
                                                    float inv, int n, float* nn_weight, int64_t* nn_idx) {
  for (int s = 0; s < K; s++) {
    float best = INFINITY; int bi = -1;
    for (int k = 0; k < B; k++) {
      if (!sel.test(k)) continue;
      const float d2 = bone_d2(bones[k], px, py, pz);
      if (d2 < best || bi < 0) { best = d2; bi = k; }
    }
    sel.reset(bi);
    if (nn_weight) nn_weight[(size_t)n * K + s] = (fast_exp(-best * bones[bi].inv2r2) + 1e-7f) * inv;
    if (nn_idx) nn_idx[(size_t)n * K + s] = bi + 1;
  }
}

#define LBS_PTS2_MIN_N 1000000
#define LBS_PTS2_MIN_J 16
// FK: the workgroup runs the kinematic chain itself (fk_device.h: ~1 us on its first wave, against a launch of its own in front
// of this one — every workgroup repeats it, workgroup 0 keeps the results)
// MAXJ = MAX_J_WIDE: skeletons of 65..256 joints — up to 255 bone records in LDS and the selection set there too; the chain is a
// launch of its own in front (riggs_lbs_forward_fk), one Gaussian per thread, weight_mod read from global memory
template <bool TOPK, bool FK, int PTS, int MAXJ = MAX_J>
__global__ __launch_bounds__(256) void lbs_forward_kernel(LbsArgs a) {
  constexpr bool WIDE = MAXJ > MAX_J;
  constexpr bool MOD_TILE = !WIDE && PTS == 1;
  static_assert(!TOPK || PTS == 1, "the top-K path takes one Gaussian per thread");
  static_assert(!WIDE || (!FK && PTS == 1 && !MOD_TILE), "beyond 64 joints: no chain inside, one Gaussian per thread, no weight_mod tile");
  typedef std::conditional_t<WIDE && TOPK, SelLds, SelReg> Sel;
  __shared__ Bone bones[MAXJ - 1];
  // (the Gaussians' positions first: their round trip runs under the chain and the staging — the compiler keeps loads behind
  // the barriers where it finds them)
  const int n0 = blockIdx.x * (256 * PTS) + threadIdx.x;
  float px[PTS], py[PTS], pz[PTS];
  bool on[PTS];
#pragma unroll
  for (int p = 0; p < PTS; p++) {
    const int n = n0 + 256 * p;
    on[p] = n < a.N;
    const int nn = min(on[p] ? n : n0, a.N - 1);
    px[p] = a.x[3 * nn]; py[p] = a.x[3 * nn + 1]; pz[p] = a.x[3 * nn + 2];
  }
  // weight_mod (WeightMLP head on): a thread reads its own row of B floats, bone by bone — as global loads that is B
  // instructions of 64 addresses 4 B bytes apart each (46 lines per instruction, the L1 thrashes: +20 us on this kernel).  The
  // wave's 64 rows are one contiguous run: copied once, coalesced, into a wave-private LDS tile (row stride odd: a column
  // read is conflict-free), where the bone loop reads them.  (a.mod_lds: the launch reserved 256 (B | 1) floats)
  [[maybe_unused]] float* s_mod = nullptr;
  [[maybe_unused]] int BP = 0;
  if constexpr (MOD_TILE) {
    extern __shared__ float s_mod_dyn[];
    BP = (a.J - 1) | 1;
    s_mod = s_mod_dyn + (threadIdx.x >> 6) * 64 * BP;
    if (a.mod_lds) {
      const int Bm = a.J - 1, lane_ = threadIdx.x & 63;
      const int ng = blockIdx.x * 256 + (threadIdx.x & ~63);
      const int n_el = max(0, min(64, a.N - ng)) * Bm;
      const float* run = a.weight_mod + (size_t)ng * Bm;
      const float invB = 1.0f / (float)Bm;
      for (int e = lane_; e < n_el; e += 64) {
        const int r = (int)(((float)e + 0.5f) * invB);
        s_mod[r * BP + (e - r * Bm)] = run[e];
      }
    }
  }
  if constexpr (FK) {
    __shared__ float G[MAX_J][12];
    __shared__ float Q[MAX_J][4];
    if (threadIdx.x < 64) {  // (wave 0: one joint per lane)
      FkIn in;
      fk_load(a.J, a.local_rot, a.joints, a.parents, nullptr, nullptr, in);
      FkLane f;
      fk_wave_forward(a.J, in, f);
      const int j = threadIdx.x;
      if (j < a.J) {
        float q[4];
        R_to_quat(f.G, q);
#pragma unroll
        for (int e = 0; e < 12; e++) G[j][e] = f.G[e];
#pragma unroll
        for (int e = 0; e < 4; e++) Q[j][e] = q[e];
        if (blockIdx.x == 0) {
          const float x = in.x[0], y = in.x[1], z = in.x[2];
#pragma unroll
          for (int e = 0; e < 12; e++) a.fk_transforms[12 * j + e] = f.G[e];
#pragma unroll
          for (int r = 0; r < 3; r++)
            a.fk_d_nodes[3 * j + r] = (f.G[4 * r] * x + f.G[4 * r + 1] * y + f.G[4 * r + 2] * z + f.G[4 * r + 3]) + a.global_trans[r];
#pragma unroll
          for (int e = 0; e < 4; e++) a.fk_node_rot[4 * j + e] = q[e];
        }
      }
    }
    __syncthreads();
    stage_bones(a, bones, &G[0][0], &Q[0][0]);
  } else {
    stage_bones(a, bones);
  }
  if constexpr (!WIDE) {
    // (the staged records for the backward, when the caller handed over a table)
    if (a.table_out && blockIdx.x == 0) for (int k = threadIdx.x; k < a.J - 1; k += 256) a.table_out[k] = bones[k];
  }
  // PTS Gaussians per thread (all-bones configuration): what bounds this loop at 64 joints is the LDS handing every wave the
  // bone records (24 floats per bone, broadcast: 8 cycles of the CU's 128 B / clk return path per ds_read_b128 and wave,
  // ~48 per bone and wave against ~26 VALU instructions per SIMD) — two Gaussians per lane read each record once for both
  // (2 M x 63: 148 -> 133 us; the kernel is then bound by vector issue: ~32 instructions per Gaussian and bone, 16 of them
  // the blend.  The blend on the matrix pipe instead — v_mfma_f32_16x16x4_f32, lane = (Gaussian i of a tile of 16, bone
  // 4 s + j): the same k-ordered fmaf chain, 19 vector instructions per pair — measured 128 us: its four dependent-free MFMAs
  // per step still cost the wave their issue, plus a transposing epilogue through LDS; not kept for 4 %).
  // (one block of 256 * PTS Gaussians per workgroup: fewer, looping workgroups — the chain and the staging above once per
  // workgroup instead of once per block — are slower: 17.5 -> 19.7 -> 24.6 us at 1172 / 586 / 293 workgroups)
  const int B = a.J - 1;
  if (n0 >= a.N) return;
  Sel sel;
  if constexpr (Sel::in_lds) {
    __shared__ typename Sel::Column s_sel;
    sel.col = s_sel;
  }
  if (TOPK) topk_select(sel, bones, B, a.K, px[0], py[0], pz[0]);
  float M[PTS][12], qa[PTS][4], sum[PTS];
#pragma unroll
  for (int p = 0; p < PTS; p++) {
    sum[p] = 0.f;
#pragma unroll
    for (int e = 0; e < 12; e++) M[p][e] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) qa[p][e] = 0.f;
  }
  for (int k = 0; k < B; k++) {
    const Bone& b = bones[k];
    if (TOPK && !sel.test(k)) continue;
#pragma unroll
    for (int p = 0; p < PTS; p++) {
      const float d2 = TOPK ? bone_d2(b, px[p], py[p], pz[p]) : bone_d2_fast(b, px[p], py[p], pz[p]);
      float u = fast_exp(-d2 * b.inv2r2);                // skeleton_warp.py:66
      if (a.weight_mod) u *= (MOD_TILE && a.mod_lds) ? s_mod[(threadIdx.x & 63) * BP + k]
                                                     : a.weight_mod[(size_t)(on[p] ? n0 + 256 * p : n0) * B + k];  // :68-69
      const float v = u + 1e-7f;                          // :71
      sum[p] += v;
#pragma unroll
      for (int e = 0; e < 12; e++) M[p][e] += v * b.G[e];
#pragma unroll
      for (int e = 0; e < 4; e++) qa[p][e] += v * b.q[e];
    }
  }
  const float gx = a.global_trans[0], gy = a.global_trans[1], gz = a.global_trans[2];
#pragma unroll
  for (int p = 0; p < PTS; p++) {
    if (!on[p]) continue;
    const int n = n0 + 256 * p;
    const float inv = 1.0f / sum[p];
    const float m = a.motion_mask ? a.motion_mask[n] : 1.0f;
    const float ax = (M[p][0] * px[p] + M[p][1] * py[p] + M[p][2] * pz[p] + M[p][3]) * inv + gx;
    const float ay = (M[p][4] * px[p] + M[p][5] * py[p] + M[p][6] * pz[p] + M[p][7]) * inv + gy;
    const float az = (M[p][8] * px[p] + M[p][9] * py[p] + M[p][10] * pz[p] + M[p][11]) * inv + gz;
    a.d_xyz[3 * n] = (ax - px[p]) * m; a.d_xyz[3 * n + 1] = (ay - py[p]) * m; a.d_xyz[3 * n + 2] = (az - pz[p]) * m;
    reinterpret_cast<float4*>(a.d_rot)[n] = make_float4(qa[p][0] * inv * m, qa[p][1] * inv * m, qa[p][2] * inv * m, qa[p][3] * inv * m);
    if (a.nn_weight || a.nn_idx) {
      if (TOPK) {
        topk_emit_ascending(sel, bones, B, a.K, px[p], py[p], pz[p], inv, n, a.nn_weight, a.nn_idx);
      } else {
        for (int k = 0; k < B; k++) {
          if (a.nn_weight) a.nn_weight[(size_t)n * B + k] = (fast_exp(-bone_d2_fast(bones[k], px[p], py[p], pz[p]) * bones[k].inv2r2) *
                                                                (a.weight_mod ? a.weight_mod[(size_t)n * B + k] : 1.0f) + 1e-7f) * inv;
          if (a.nn_idx) a.nn_idx[(size_t)n * B + k] = k + 1;
        }
      }
    }
  }
}

// ---- the all-bones forward with the bone records in SGPRs (large scenes; riggs_set_option("lbs_scalar")).  A bone
// record is the same for every lane: here it comes from a table in global memory through the scalar cache (the constant address
// space makes the uniform loads s_load_dwordx8 / x4) and feeds the vector instructions as scalar operands — no LDS image, no
// barrier, no ds_read_b128 broadcast per bone and wave; the results are bit-identical to the LDS form's (same operations, same
// order).  The table (the staged Bone records) is written by a one-workgroup launch in front: chosen by lbs_use_scalar.
__global__ __launch_bounds__(64) void lbs_bone_table_kernel(LbsArgs a, Bone* __restrict__ table) {
  __shared__ Bone bones[MAX_J - 1];
  stage_bones(a, bones);
  for (int k = threadIdx.x; k < a.J - 1; k += 64) table[k] = bones[k];
}
// ... and with the kinematic chain in front of it (riggs_lbs_forward_fk's large-scene form): one wave runs the chain, leaves its
// results where the backward reads them, and the table
__global__ __launch_bounds__(64) void lbs_fk_table_kernel(LbsArgs a, Bone* __restrict__ table) {
  __shared__ Bone bones[MAX_J - 1];
  __shared__ float G[MAX_J][12];
  __shared__ float Q[MAX_J][4];
  FkIn in;
  fk_load(a.J, a.local_rot, a.joints, a.parents, nullptr, nullptr, in);
  FkLane f;
  fk_wave_forward(a.J, in, f);
  const int j = threadIdx.x;
  if (j < a.J) {
    float q[4];
    R_to_quat(f.G, q);
    const float x = in.x[0], y = in.x[1], z = in.x[2];
#pragma unroll
    for (int e = 0; e < 12; e++) { G[j][e] = f.G[e]; a.fk_transforms[12 * j + e] = f.G[e]; }
#pragma unroll
    for (int r = 0; r < 3; r++)
      a.fk_d_nodes[3 * j + r] = (f.G[4 * r] * x + f.G[4 * r + 1] * y + f.G[4 * r + 2] * z + f.G[4 * r + 3]) + a.global_trans[r];
#pragma unroll
    for (int e = 0; e < 4; e++) { Q[j][e] = q[e]; a.fk_node_rot[4 * j + e] = q[e]; }
  }
  __syncthreads();
  stage_bones(a, bones, &G[0][0], &Q[0][0]);
  for (int k = threadIdx.x; k < a.J - 1; k += 64) table[k] = bones[k];
}
typedef __attribute__((address_space(4))) const Bone* LbsConstBones;
template <int PTS>
__global__ __launch_bounds__(256) void lbs_forward_scalar_kernel(LbsArgs a, const Bone* __restrict__ table_g) {
  const LbsConstBones table = (LbsConstBones)table_g;
  const int n0 = blockIdx.x * (256 * PTS) + threadIdx.x;
  float px[PTS], py[PTS], pz[PTS];
  bool on[PTS];
#pragma unroll
  for (int p = 0; p < PTS; p++) {
    const int n = n0 + 256 * p;
    on[p] = n < a.N;
    const int nn = min(on[p] ? n : n0, a.N - 1);
    px[p] = a.x[3 * nn]; py[p] = a.x[3 * nn + 1]; pz[p] = a.x[3 * nn + 2];
  }
  const int B = a.J - 1;
  if (n0 >= a.N) return;
  float M[PTS][12], qa[PTS][4], sum[PTS];
#pragma unroll
  for (int p = 0; p < PTS; p++) {
    sum[p] = 0.f;
#pragma unroll
    for (int e = 0; e < 12; e++) M[p][e] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) qa[p][e] = 0.f;
  }
  for (int k = 0; k < B; k++) {
    const float a0 = table[k].a[0], a1 = table[k].a[1], a2 = table[k].a[2];
    const float b0 = table[k].ba[0], b1 = table[k].ba[1], b2 = table[k].ba[2];
    const float rl2 = table[k].rl2, i2r = table[k].inv2r2;
    float G[12], q[4];
#pragma unroll
    for (int e = 0; e < 12; e++) G[e] = table[k].G[e];
#pragma unroll
    for (int e = 0; e < 4; e++) q[e] = table[k].q[e];
#pragma unroll
    for (int p = 0; p < PTS; p++) {
      const float ex = px[p] - a0, ey = py[p] - a1, ez = pz[p] - a2;
      const float t = __builtin_amdgcn_fmed3f((ex * b0 + ey * b1 + ez * b2) * rl2, 0.0f, 1.0f);
      const float sx = t * b0 - ex, sy = t * b1 - ey, sz = t * b2 - ez;
      const float d2 = sx * sx + sy * sy + sz * sz;
      float u = fast_exp(-d2 * i2r);
      if (a.weight_mod) u *= a.weight_mod[(size_t)(on[p] ? n0 + 256 * p : n0) * B + k];
      const float v = u + 1e-7f;
      sum[p] += v;
#pragma unroll
      for (int e = 0; e < 12; e++) M[p][e] += v * G[e];
#pragma unroll
      for (int e = 0; e < 4; e++) qa[p][e] += v * q[e];
    }
  }
  const float gx = a.global_trans[0], gy = a.global_trans[1], gz = a.global_trans[2];
#pragma unroll
  for (int p = 0; p < PTS; p++) {
    if (!on[p]) continue;
    const int n = n0 + 256 * p;
    const float inv = 1.0f / sum[p];
    const float m = a.motion_mask ? a.motion_mask[n] : 1.0f;
    const float ax = (M[p][0] * px[p] + M[p][1] * py[p] + M[p][2] * pz[p] + M[p][3]) * inv + gx;
    const float ay = (M[p][4] * px[p] + M[p][5] * py[p] + M[p][6] * pz[p] + M[p][7]) * inv + gy;
    const float az = (M[p][8] * px[p] + M[p][9] * py[p] + M[p][10] * pz[p] + M[p][11]) * inv + gz;
    a.d_xyz[3 * n] = (ax - px[p]) * m; a.d_xyz[3 * n + 1] = (ay - py[p]) * m; a.d_xyz[3 * n + 2] = (az - pz[p]) * m;
    reinterpret_cast<float4*>(a.d_rot)[n] = make_float4(qa[p][0] * inv * m, qa[p][1] * inv * m, qa[p][2] * inv * m, qa[p][3] * inv * m);
  }
}

// Backward.  Per bone 13 sums over the Gaussians: dG_k (12) = sum_n w_nk * (ghat_n (x) [x_n;1]) and
// drho_k = sum_n dL/dv_nk * u_nk * d2_nk * exp(-2 rho_k).
// This thread-per-Gaussian kernel serves the top-K configuration (K > 0, skeleton_warp.py:46-49: every Gaussian has its
// own bone subset); the all-bones default (K = -1) runs the bone-lane kernel below.
// (K > 0 is required: with K <= 0 the selection would be empty.  The host launches it for K > 0 only.)
__global__ __launch_bounds__(256) void lbs_backward_kernel(LbsArgs a) {
  __shared__ Bone bones[MAX_J - 1];
  __shared__ float s_acc[MAX_J - 1][13];
  __shared__ float s_gt[3];
  SelReg sel;
  stage_bones(a, bones);
  const int B = a.J - 1;
  for (int e = threadIdx.x; e < B * 13; e += 256) (&s_acc[0][0])[e] = 0.f;
  if (threadIdx.x < 3) s_gt[threadIdx.x] = 0.f;
  __syncthreads();
  const int n = blockIdx.x * 256 + threadIdx.x;
  const bool valid = n < a.N;
  const int lane = threadIdx.x & 63;
  float px = 0.f, py = 0.f, pz = 0.f, m = 0.f;
  float g[3] = {0.f, 0.f, 0.f}, h[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid) {
    px = a.x[3 * n]; py = a.x[3 * n + 1]; pz = a.x[3 * n + 2];
    m = a.motion_mask ? a.motion_mask[n] : 1.0f;
    g[0] = a.g_xyz[3 * n]; g[1] = a.g_xyz[3 * n + 1]; g[2] = a.g_xyz[3 * n + 2];
    const float4 hh = reinterpret_cast<const float4*>(a.g_rot)[n];
    h[0] = hh.x; h[1] = hh.y; h[2] = hh.z; h[3] = hh.w;
  }
  const float gh[3] = {g[0] * m, g[1] * m, g[2] * m};
  const float hh4[4] = {h[0] * m, h[1] * m, h[2] * m, h[3] * m};
  // pass 1: normaliser and blended outputs
  topk_select(sel, bones, B, a.K, px, py, pz);
  float M[12], qa[4] = {0.f, 0.f, 0.f, 0.f}, sum = 0.f;
#pragma unroll
  for (int e = 0; e < 12; e++) M[e] = 0.f;
  for (int k = 0; k < B; k++) {
    const Bone& b = bones[k];
    if (!sel.test(k)) continue;
    const float d2 = bone_d2(b, px, py, pz);
    const float v = fast_exp(-d2 * b.inv2r2) + 1e-7f;
    sum += v;
#pragma unroll
    for (int e = 0; e < 12; e++) M[e] += v * b.G[e];
#pragma unroll
    for (int e = 0; e < 4; e++) qa[e] += v * b.q[e];
  }
  const float inv = valid ? 1.0f / sum : 0.f;
  const float ax = (M[0] * px + M[1] * py + M[2] * pz + M[3]) * inv;
  const float ay = (M[4] * px + M[5] * py + M[6] * pz + M[7]) * inv;
  const float az = (M[8] * px + M[9] * py + M[10] * pz + M[11]) * inv;
  const float qv[4] = {qa[0] * inv, qa[1] * inv, qa[2] * inv, qa[3] * inv};
  // S = sum_j w_j dL/dw_j
  const float S = gh[0] * ax + gh[1] * ay + gh[2] * az + hh4[0] * qv[0] + hh4[1] * qv[1] + hh4[2] * qv[2] + hh4[3] * qv[3];
  if (valid && a.dmask) {
    const float gxs = a.global_trans[0], gys = a.global_trans[1], gzs = a.global_trans[2];
    a.dmask[n] = g[0] * (ax + gxs - px) + g[1] * (ay + gys - py) + g[2] * (az + gzs - pz) + h[0] * qv[0] + h[1] * qv[1] +
                 h[2] * qv[2] + h[3] * qv[3];
  }
  // pass 2: per-bone contributions, reduced over the wave
  const float P[12] = {gh[0] * px, gh[0] * py, gh[0] * pz, gh[0], gh[1] * px, gh[1] * py, gh[1] * pz, gh[1],
                       gh[2] * px, gh[2] * py, gh[2] * pz, gh[2]};
  for (int k = 0; k < B; k++) {
    const bool sel_k = sel.test(k);
    const Bone& b = bones[k];
    const float d2 = bone_d2(b, px, py, pz);
    float w = 0.f, r = 0.f;
    if (valid && sel_k) {
      const float u = fast_exp(-d2 * b.inv2r2);
      w = (u + 1e-7f) * inv;
      const float Ax = b.G[0] * px + b.G[1] * py + b.G[2] * pz + b.G[3];
      const float Ay = b.G[4] * px + b.G[5] * py + b.G[6] * pz + b.G[7];
      const float Az = b.G[8] * px + b.G[9] * py + b.G[10] * pz + b.G[11];
      const float dLdw = gh[0] * Ax + gh[1] * Ay + gh[2] * Az + hh4[0] * b.q[0] + hh4[1] * b.q[1] + hh4[2] * b.q[2] + hh4[3] * b.q[3];
      const float dLdv = (dLdw - S) * inv;
      r = dLdv * u * d2 * (2.0f * b.inv2r2);
    }
    float red[13];
#pragma unroll
    for (int e = 0; e < 12; e++) red[e] = wave_sum(w * P[e]);
    red[12] = wave_sum(r);
    if (lane == 63) {
#pragma unroll
      for (int e = 0; e < 13; e++) atomicAdd(&s_acc[k][e], red[e]);
    }
  }
  const float t0 = wave_sum(gh[0]), t1 = wave_sum(gh[1]), t2 = wave_sum(gh[2]);
  if (lane == 63) { atomicAdd(&s_gt[0], t0); atomicAdd(&s_gt[1], t1); atomicAdd(&s_gt[2], t2); }
  __syncthreads();
  for (int e = threadIdx.x; e < B * 13; e += 256) {
    const int k = e / 13, c = e % 13;
    const float v = s_acc[k][c];
    if (c < 12) atomicAdd(&a.dG[12 * (k + 1) + c], v);
    else atomicAdd(&a.drho[k + 1], v);
  }
  if (threadIdx.x < 3) atomicAdd(&a.dgt[threadIdx.x], s_gt[threadIdx.x]);
}

// ---- backward, K <= 0 (all bones): lane <-> (Gaussian slot, bone) ---------------------------------
// A wave64 is 8 Gaussian slots x 8 bone lanes; bones are covered in blocks of 8.  Each lane owns one
// bone per block, so the 13 per-bone sums over the Gaussians are plain register accumulations (no
// cross-lane reduction per Gaussian); only the two per-Gaussian normalisers (sum_k v_k and
// sum_k v_k dL/dw_k) are reduced over the 8 bone lanes (3 DPP steps).  The 8 slot rows are folded once
// per wave at the end.  (The pixel-major variant above spent ~30 DPP ops per (Gaussian, bone).)
#define LB_BONES 8                      // bone lanes per Gaussian slot
#define LB_MAXBLK ((MAX_J - 1 + LB_BONES - 1) / LB_BONES)
#ifndef LB_GPB
#define LB_GPB 1024                     // Gaussians per workgroup: every wave looks at a quarter of them, 64 at a time
#endif

__device__ __forceinline__ float row8_sum(float v) {
  // sum over the 8 lanes sharing (lane >> 3): xor 1, 2, 4 via DPP quad_perm / row_half_mirror patterns
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));  // row_half_mirror
  return v;
}

// The prologue of the <= 64-joint kernel (one walk) and of the 65..256-joint one (passes of LBW_PASS blocks):
// stage the bones; padding bones up to nb blocks (never selected); zero the workgroup's sums
__device__ __forceinline__ void lbs_bonelane_prologue(const LbsArgs& a, Bone* bones, float (*s_acc)[13], float* s_gt, int nb) {
  const int B = a.J - 1;
  stage_bones(a, bones);
  for (int k = B + threadIdx.x; k < nb * LB_BONES; k += 256) {  // padding bones: never selected
    Bone z;
    memset(&z, 0, sizeof(z));
    z.len2c = 1.f;
    bones[k] = z;
  }
  for (int e = threadIdx.x; e < nb * LB_BONES * 13; e += 256) (&s_acc[0][0])[e] = 0.f;
  if (threadIdx.x < 3) s_gt[threadIdx.x] = 0.f;
  __syncthreads();
}
template <int NBLK, bool MOD, int GPB>
__global__ __launch_bounds__(256) void lbs_backward_bonelane_kernel(LbsArgs a) {
  __shared__ Bone bones[MAX_J - 1 + LB_BONES];
  // (a slot per wave: the four waves' sums meet in wave order, so the workgroup's partial — and with the fixed-order second stage
  // every gradient of the call — is the same to the bit from run to run)
  __shared__ float s_acc[4][MAX_J - 1 + LB_BONES][13];
  __shared__ float s_gt[4][3];
  const int B = a.J - 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane >> 3, bl = lane & 7;
  const int wave_first = blockIdx.x * GPB + wave * (GPB / 4);
  const int wave_end = min(a.N, wave_first + GPB / 4);
  // Gaussians without an incoming gradient (behind saturated pixels, never at alpha >= 1/255, invisible: most of a
  // deep scene) contribute exact zeros to every sum: the wave looks at its Gaussians once, writes the zeros of
  // the per-Gaussian outputs, and walks only the others, eight at a time.
  // The wave's Gaussians are looked at in batches of four groups of 64 — their loads in flight together — and the ones with a
  // gradient are listed across the groups: walking group by group paid two dependent round trips (test, then the listed
  // Gaussians' operands) per group, which was most of this kernel's time in a sparse frame.  The FIRST batch is requested
  // before the bones are staged: its round trip runs under theirs.
  // (a large scene's workgroups take four or eight times the Gaussians — GPB = 4096 / 8192: the bones' staging, the fold of
  // the sums and the partials cost a workgroup ~15 us whatever it walks)
  constexpr int GROUPS = GPB / 4 / 64, GBATCH = 4;
  float4 hq[GBATCH];
  float gq[GBATCH][3];
  auto request = [&](const int gb) {
#pragma unroll
    for (int g4 = 0; g4 < GBATCH; g4++) {
      const int n = wave_first + 64 * (gb + g4) + lane;
      hq[g4] = make_float4(0.f, 0.f, 0.f, 0.f); gq[g4][0] = 0.f; gq[g4][1] = 0.f; gq[g4][2] = 0.f;
      if (n < wave_end) {
        hq[g4] = reinterpret_cast<const float4*>(a.g_rot)[n];
        gq[g4][0] = a.g_xyz[3 * n]; gq[g4][1] = a.g_xyz[3 * n + 1]; gq[g4][2] = a.g_xyz[3 * n + 2];
      }
    }
  };
  request(0);
  lbs_bonelane_prologue(a, bones, s_acc[0], s_gt[0], NBLK);
  float acc[NBLK][13];
#pragma unroll
  for (int bb = 0; bb < NBLK; bb++)
#pragma unroll
    for (int e = 0; e < 13; e++) acc[bb][e] = 0.f;
  float gt0 = 0.f, gt1 = 0.f, gt2 = 0.f;
  const float gx = a.global_trans[0], gy = a.global_trans[1], gz = a.global_trans[2];
  __shared__ unsigned short s_list[4][GPB / 4];
  int n_work = 0;
#pragma unroll 1
  for (int gb = 0; gb < GROUPS; gb += GBATCH) {
    if (gb > 0) request(gb);
#pragma unroll
    for (int g4 = 0; g4 < GBATCH; g4++) {
      const int n = wave_first + 64 * (gb + g4) + lane;
      const bool touched = (gq[g4][0] != 0.f) || (gq[g4][1] != 0.f) || (gq[g4][2] != 0.f) ||
                           (hq[g4].x != 0.f) || (hq[g4].y != 0.f) || (hq[g4].z != 0.f) || (hq[g4].w != 0.f);
      if (n < wave_end && !touched && a.dmask) a.dmask[n] = 0.f;
      const uint64_t tm = __builtin_amdgcn_ballot_w64(touched);
      if constexpr (MOD) {
        // the zeros of dL/dweight_mod for the group's untouched rows: the group's 64 rows are ONE contiguous run of 64 B floats —
        // 16-byte pieces, consecutive lanes = consecutive addresses (a row of B floats per lane was B stores of 64 scattered
        // dwords each: 46 partially written lines per instruction, +29 us on this kernel with the WeightMLP on); a piece that
        // overlaps a touched row (the walk below writes those) is written element by element
        const int ng = wave_first + 64 * (gb + g4);
        const int n_el = max(0, min(64, wave_end - ng)) * B;
        float* run = a.dmod + (size_t)ng * B;
        const float invB = 1.0f / (float)B;
        for (int p4 = lane * 4; p4 < n_el; p4 += 256) {
          const int r0 = (int)(((float)p4 + 0.5f) * invB), r1 = (int)(((float)min(p4 + 3, n_el - 1) + 0.5f) * invB);
          if (p4 + 3 < n_el && !((tm >> r0) & 1ull) && !((tm >> r1) & 1ull)) {
            *reinterpret_cast<float4*>(run + p4) = make_float4(0.f, 0.f, 0.f, 0.f);
          } else {
#pragma unroll
            for (int q = 0; q < 4; q++) {
              const int e = p4 + q;
              if (e < n_el && !((tm >> (int)(((float)e + 0.5f) * invB)) & 1ull)) run[e] = 0.f;
            }
          }
        }
      }
      if (touched) s_list[wave][n_work + __builtin_popcountll(tm & ((1ull << lane) - 1ull))] = (unsigned short)(64 * (gb + g4) + lane);
      n_work += __builtin_popcountll(tm);
    }
  }
  {
  const int sub_first = wave_first;
  // operands of a step's eight Gaussians, requested one step ahead of their use
  struct StepOps { int n; bool valid; float px, py, pz, m, g0, g1, g2; float4 h; };
  auto fetch = [&](int w0) {
    StepOps o;
    o.valid = w0 + slot < n_work;
    o.n = o.valid ? sub_first + (int)s_list[wave][w0 + slot] : 0;  // (a wave's own LDS writes are ordered)
    o.px = 0.f; o.py = 0.f; o.pz = 0.f; o.m = 0.f; o.g0 = 0.f; o.g1 = 0.f; o.g2 = 0.f;
    o.h = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o.valid) {
      o.px = a.x[3 * o.n]; o.py = a.x[3 * o.n + 1]; o.pz = a.x[3 * o.n + 2];
      o.m = a.motion_mask ? a.motion_mask[o.n] : 1.0f;
      o.g0 = a.g_xyz[3 * o.n]; o.g1 = a.g_xyz[3 * o.n + 1]; o.g2 = a.g_xyz[3 * o.n + 2];
      o.h = reinterpret_cast<const float4*>(a.g_rot)[o.n];
    }
    return o;
  };
  StepOps nxt = fetch(0);
  for (int w0 = 0; w0 < n_work; w0 += 8) {
    const StepOps cu = nxt;
    if (w0 + 8 < n_work) nxt = fetch(w0 + 8);
    const bool valid = cu.valid;
    const int n = cu.n;
    const float px = cu.px, py = cu.py, pz = cu.pz, m = cu.m, g0 = cu.g0, g1 = cu.g1, g2 = cu.g2;
    const float4 h = cu.h;
    const float gh0 = g0 * m, gh1 = g1 * m, gh2 = g2 * m;
    const float hh0 = h.x * m, hh1 = h.y * m, hh2 = h.z * m, hh3 = h.w * m;
    // pass 1: this lane's bones
    float v[NBLK], u[NBLK], d2[NBLK], dw[NBLK], du[NBLK], md[NBLK];
    float sum = 0.f, sv = 0.f, su = 0.f;
#pragma unroll
    for (int bb = 0; bb < NBLK; bb++) {
      const int k = bb * LB_BONES + bl;
      const Bone& b = bones[k];
      d2[bb] = bone_d2_fast(b, px, py, pz);
      const bool on = valid && (k < B);
      u[bb] = on ? fast_exp(-d2[bb] * b.inv2r2) : 0.f;
      if constexpr (MOD) {
        md[bb] = on ? a.weight_mod[(size_t)n * B + k] : 1.0f;
        v[bb] = on ? u[bb] * md[bb] + 1e-7f : 0.f;
      } else {
        md[bb] = 1.0f;
        v[bb] = on ? u[bb] + 1e-7f : 0.f;
      }
      const float Ax = b.G[0] * px + b.G[1] * py + b.G[2] * pz + b.G[3];
      const float Ay = b.G[4] * px + b.G[5] * py + b.G[6] * pz + b.G[7];
      const float Az = b.G[8] * px + b.G[9] * py + b.G[10] * pz + b.G[11];
      dw[bb] = gh0 * Ax + gh1 * Ay + gh2 * Az + hh0 * b.q[0] + hh1 * b.q[1] + hh2 * b.q[2] + hh3 * b.q[3];
      du[bb] = g0 * Ax + g1 * Ay + g2 * Az + h.x * b.q[0] + h.y * b.q[1] + h.z * b.q[2] + h.w * b.q[3];  // un-masked (dmask)
      sum += v[bb];
      sv += v[bb] * dw[bb];
      su += v[bb] * du[bb];
    }
    sum = row8_sum(sum);
    sv = row8_sum(sv);
    const float inv = valid ? 1.0f / sum : 0.f;
    const float S = sv * inv;
    if (a.dmask) {
      su = row8_sum(su);
      if (valid && bl == 0) a.dmask[n] = su * inv + g0 * (gx - px) + g1 * (gy - py) + g2 * (gz - pz);
    }
    // pass 2: accumulate this lane's bones
    const float P[12] = {gh0 * px, gh0 * py, gh0 * pz, gh0, gh1 * px, gh1 * py, gh1 * pz, gh1,
                         gh2 * px, gh2 * py, gh2 * pz, gh2};
#pragma unroll
    for (int bb = 0; bb < NBLK; bb++) {
      const float w = v[bb] * inv;
      const float dLdv = (dw[bb] - S) * inv;
      float r;
      if constexpr (MOD) r = dLdv * md[bb] * u[bb] * d2[bb] * (2.0f * bones[bb * LB_BONES + bl].inv2r2);
      else r = dLdv * u[bb] * d2[bb] * (2.0f * bones[bb * LB_BONES + bl].inv2r2);
      if (MOD && valid && bb * LB_BONES + bl < B) a.dmod[(size_t)n * B + bb * LB_BONES + bl] = dLdv * u[bb];  // v = u * mod + 1e-7
#pragma unroll
      for (int e = 0; e < 12; e++) acc[bb][e] += w * P[e];
      acc[bb][12] += r;
    }
    if (bl == 0) { gt0 += gh0; gt1 += gh1; gt2 += gh2; }
  }
  }
  // fold the 8 slot rows (lanes l, l^8, l^16, l^32) and leave them in the wave's slot of the workgroup accumulators (a wave
  // writes every entry of its slot, zeros where it walked nothing)
#pragma unroll
  for (int bb = 0; bb < NBLK; bb++)
#pragma unroll
    for (int e = 0; e < 13; e++) {
      float t = acc[bb][e];
      t += __shfl_xor(t, 8); t += __shfl_xor(t, 16); t += __shfl_xor(t, 32);
      if (slot == 0) s_acc[wave][bb * LB_BONES + bl][e] = t;
    }
  gt0 = wave_sum(gt0); gt1 = wave_sum(gt1); gt2 = wave_sum(gt2);
  if (lane == 63) { s_gt[wave][0] = gt0; s_gt[wave][1] = gt1; s_gt[wave][2] = gt2; }
  __syncthreads();
  // per-workgroup partial sums: the waves' slots added in wave order (as the LDS atomics that used to meet here did when the waves
  // arrived in that order; in any other order the last place of dG / drho / dgt differed from run to run from three contributing
  // waves on — N > 512); lbs_backward_finish_kernel adds the partials up in a fixed order too
  float* part = a.partial + (size_t)blockIdx.x * (B * 13 + 3);
  for (int e = threadIdx.x; e < B * 13; e += 256)
    part[e] = (((0.f + (&s_acc[0][0][0])[e]) + (&s_acc[1][0][0])[e]) + (&s_acc[2][0][0])[e]) + (&s_acc[3][0][0])[e];
  if (threadIdx.x < 3)
    part[B * 13 + threadIdx.x] = (((0.f + s_gt[0][threadIdx.x]) + s_gt[1][threadIdx.x]) + s_gt[2][threadIdx.x]) + s_gt[3][threadIdx.x];
}

// one workgroup per output value: sum over the workgroups' partials
__global__ __launch_bounds__(256) void lbs_backward_finish_kernel(LbsArgs a, int n_parts) {
  __shared__ float s_red[4];
  const int B = a.J - 1, stride = B * 13 + 3, e = blockIdx.x;
  float t = 0.f;
  for (int p = threadIdx.x; p < n_parts; p += 256) t += a.partial[(size_t)p * stride + e];
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 63) s_red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    if (e < B * 13) {
      const int k = e / 13, c = e % 13;
      if (c < 12) a.dG[12 * (k + 1) + c] = v; else a.drho[k + 1] = v;
    } else a.dgt[e - B * 13] = v;
  }
  // joint 0 carries no bone: its transform / radius receive no gradient from the skinning
  if (e == 0 && threadIdx.x < 12) a.dG[threadIdx.x] = 0.f;
  if (e == 0 && threadIdx.x == 12) a.drho[0] = 0.f;
}

template <int NBLK, int GPB>
static void launch_lbs_bwd_bonelane_g(const LbsArgs& a, hipStream_t s) {
  const int blocks = (a.N + GPB - 1) / GPB;
  // (the weight-modulated variant — WeightMLP head on — is a separate instantiation: the LBS-only kernel keeps its registers)
  if (a.weight_mod) hipLaunchKernelGGL((lbs_backward_bonelane_kernel<NBLK, true, GPB>), dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((lbs_backward_bonelane_kernel<NBLK, false, GPB>), dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(lbs_backward_finish_kernel, dim3((a.J - 1) * 13 + 3), dim3(256), 0, s, a, blocks);
}
template <int NBLK>
static void launch_lbs_bwd_bonelane(const LbsArgs& a, hipStream_t s) {
  // 1024 Gaussians per workgroup fill the chip at the bench size (293 workgroups).  At 64 joints the kernel holds 13 sums for
  // 8 blocks of bones per lane — 256 VGPRs, ONE workgroup per CU — and a workgroup costs ~15 us whatever it walks (staging
  // the bones, the fold of the sums, the partials): 2 M Gaussians were 1954 workgroups = 7.6 rounds = 154 us.  So a large
  // scene's workgroups take as many Gaussians as leave about one workgroup per CU.
  if (a.N >= 8 * 240 * 1024) launch_lbs_bwd_bonelane_g<NBLK, 8192>(a, s);
  else if (a.N >= 4 * 240 * 1024) launch_lbs_bwd_bonelane_g<NBLK, 4096>(a, s);
  else launch_lbs_bwd_bonelane_g<NBLK, LB_GPB>(a, s);
}

// ==================================================================================== skeletons of 65..256 joints
// The chain on one workgroup (fk_device.h: fk_block_*), and the bone-lane backward walking the bones in passes of 64, are
// kernels of their own, and so is the top-K backward; the skinning forward is the MAX_J_WIDE instantiation of the template above
// (up to 255 bone records in LDS, the top-K selection set as 256 bits per thread in LDS: SelLds).  The <= 64-joint
// instantiations keep their LDS footprint, registers and occupancy.
#define MAX_B_WIDE (MAX_J_WIDE - 1)

__global__ __launch_bounds__(256) void fk_forward_wide_kernel(int J, const float* __restrict__ local_rot,
                                                              const float* __restrict__ joints,
                                                              const int32_t* __restrict__ parents,
                                                              const float* __restrict__ global_trans,
                                                              float* __restrict__ transforms, float* __restrict__ node_rot,
                                                              float* __restrict__ d_nodes) {
  __shared__ FkWideShared sh;
  const int j = threadIdx.x;
  FkIn in;
  fk_load_joint(j, J, local_rot, joints, parents, nullptr, nullptr, in);
  FkWide f;
  fk_block_forward(J, in, f, sh);
  if (j < J) {
    float G[12];
#pragma unroll
    for (int e = 0; e < 12; e++) G[e] = sh.G[j][e];
    const float x = in.x[0], y = in.x[1], z = in.x[2];
#pragma unroll
    for (int e = 0; e < 12; e++) transforms[12 * j + e] = G[e];
#pragma unroll
    for (int r = 0; r < 3; r++)
      d_nodes[3 * j + r] = (G[4 * r] * x + G[4 * r + 1] * y + G[4 * r + 2] * z + G[4 * r + 3]) + global_trans[r];
    float q[4];
    R_to_quat(G, q);
#pragma unroll
    for (int e = 0; e < 4; e++) node_rot[4 * j + e] = q[e];
  }
}

__global__ __launch_bounds__(256) void fk_backward_wide_kernel(int J, const float* __restrict__ local_rot,
                                                               const float* __restrict__ joints,
                                                               const int32_t* __restrict__ parents,
                                                               const float* __restrict__ dL_dG_in,
                                                               const float* __restrict__ dL_dnodes,
                                                               float* __restrict__ dL_dlocal_rot,
                                                               float* __restrict__ dL_dglobal_trans) {
  __shared__ FkWideShared sh;
  const int j = threadIdx.x;
  FkIn in;
  fk_load_joint(j, J, local_rot, joints, parents, dL_dG_in, dL_dnodes, in);
  FkWide f;
  fk_block_forward(J, in, f, sh);
  if (dL_dnodes && j < 3) {  // d_nodes = posed + global_trans
    float s = 0.f;
    for (int k = 0; k < J; k++) s += dL_dnodes[3 * k + j];
    dL_dglobal_trans[j] += s;
  }
  float dq[4];
  fk_block_backward(J, in, f, sh, dq);
  if (j < J) {
#pragma unroll
    for (int e = 0; e < 4; e++) dL_dlocal_rot[4 * j + e] = dq[e];
  }
}

// topk_mask over up to 255 bones: the same K passes in the same (d2, index) order, the thread's 256-bit mask a column of
// `sel` in LDS (word w of thread t at sel[w][t]: conflict-free)
typedef SelLds::Column SelWide;
__device__ __forceinline__ void topk_mask_wide(const Bone* bones, int B, int K, float px, float py, float pz, SelWide& sel) {
  const int t = threadIdx.x;
#pragma unroll
  for (int w = 0; w < FK_WIDE_WORDS; w++) sel[w][t] = 0u;
  for (int s = 0; s < K; s++) {
    float best = INFINITY;
    int bi = -1;
    uint32_t m = 0u;
    for (int k = 0; k < B; k++) {
      if ((k & 31) == 0) m = sel[k >> 5][t];
      if ((m >> (k & 31)) & 1u) continue;
      const float d2 = bone_d2(bones[k], px, py, pz);
      if (d2 < best || bi < 0) { best = d2; bi = k; }
    }
    sel[bi >> 5][t] |= 1u << (bi & 31);
  }
}

// lbs_backward_kernel (top-K, thread per Gaussian) for J > 64: a kernel of its own, with its own K selection passes.  As the
// LDS-column instantiation of one template with lbs_backward_kernel (SelLds, topk_select) it measured 0.9 % slower on the
// MI355X at 128 and 256 joints (300 k Gaussians, K = 3: 592.6 -> 597.9 us, 1106.5 -> 1116.6 us, outside the spread of
// five repeats), so the two stay apart.
__global__ __launch_bounds__(256) void lbs_backward_wide_kernel(LbsArgs a) {
  __shared__ Bone bones[MAX_B_WIDE];
  __shared__ float s_acc[MAX_B_WIDE][13];
  __shared__ SelWide s_sel;
  __shared__ float s_gt[3];
  stage_bones(a, bones);
  const int B = a.J - 1, t = threadIdx.x;
  for (int e = t; e < B * 13; e += 256) (&s_acc[0][0])[e] = 0.f;
  if (t < 3) s_gt[t] = 0.f;
  __syncthreads();
  const int n = blockIdx.x * 256 + t;
  const bool valid = n < a.N;
  const int lane = t & 63;
  float px = 0.f, py = 0.f, pz = 0.f, m = 0.f;
  float g[3] = {0.f, 0.f, 0.f}, h[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid) {
    px = a.x[3 * n]; py = a.x[3 * n + 1]; pz = a.x[3 * n + 2];
    m = a.motion_mask ? a.motion_mask[n] : 1.0f;
    g[0] = a.g_xyz[3 * n]; g[1] = a.g_xyz[3 * n + 1]; g[2] = a.g_xyz[3 * n + 2];
    const float4 hh = reinterpret_cast<const float4*>(a.g_rot)[n];
    h[0] = hh.x; h[1] = hh.y; h[2] = hh.z; h[3] = hh.w;
  }
  const float gh[3] = {g[0] * m, g[1] * m, g[2] * m};
  const float hh4[4] = {h[0] * m, h[1] * m, h[2] * m, h[3] * m};
  // pass 1: normaliser and blended outputs
  topk_mask_wide(bones, B, a.K, px, py, pz, s_sel);
  float M[12], qa[4] = {0.f, 0.f, 0.f, 0.f}, sum = 0.f;
#pragma unroll
  for (int e = 0; e < 12; e++) M[e] = 0.f;
  uint32_t sm = 0u;
  for (int k = 0; k < B; k++) {
    if ((k & 31) == 0) sm = s_sel[k >> 5][t];
    if (!((sm >> (k & 31)) & 1u)) continue;
    const Bone& b = bones[k];
    const float d2 = bone_d2(b, px, py, pz);
    const float v = fast_exp(-d2 * b.inv2r2) + 1e-7f;
    sum += v;
#pragma unroll
    for (int e = 0; e < 12; e++) M[e] += v * b.G[e];
#pragma unroll
    for (int e = 0; e < 4; e++) qa[e] += v * b.q[e];
  }
  const float inv = valid ? 1.0f / sum : 0.f;
  const float ax = (M[0] * px + M[1] * py + M[2] * pz + M[3]) * inv;
  const float ay = (M[4] * px + M[5] * py + M[6] * pz + M[7]) * inv;
  const float az = (M[8] * px + M[9] * py + M[10] * pz + M[11]) * inv;
  const float qv[4] = {qa[0] * inv, qa[1] * inv, qa[2] * inv, qa[3] * inv};
  const float S = gh[0] * ax + gh[1] * ay + gh[2] * az + hh4[0] * qv[0] + hh4[1] * qv[1] + hh4[2] * qv[2] + hh4[3] * qv[3];
  if (valid && a.dmask) {
    const float gxs = a.global_trans[0], gys = a.global_trans[1], gzs = a.global_trans[2];
    a.dmask[n] = g[0] * (ax + gxs - px) + g[1] * (ay + gys - py) + g[2] * (az + gzs - pz) + h[0] * qv[0] + h[1] * qv[1] +
                 h[2] * qv[2] + h[3] * qv[3];
  }
  // pass 2: per-bone contributions, reduced over the wave
  const float P[12] = {gh[0] * px, gh[0] * py, gh[0] * pz, gh[0], gh[1] * px, gh[1] * py, gh[1] * pz, gh[1],
                       gh[2] * px, gh[2] * py, gh[2] * pz, gh[2]};
  for (int k = 0; k < B; k++) {
    if ((k & 31) == 0) sm = s_sel[k >> 5][t];
    const Bone& b = bones[k];
    const float d2 = bone_d2(b, px, py, pz);
    float w = 0.f, r = 0.f;
    const bool sel = valid && ((sm >> (k & 31)) & 1u);
    if (sel) {
      const float u = fast_exp(-d2 * b.inv2r2);
      w = (u + 1e-7f) * inv;
      const float Ax = b.G[0] * px + b.G[1] * py + b.G[2] * pz + b.G[3];
      const float Ay = b.G[4] * px + b.G[5] * py + b.G[6] * pz + b.G[7];
      const float Az = b.G[8] * px + b.G[9] * py + b.G[10] * pz + b.G[11];
      const float dLdw = gh[0] * Ax + gh[1] * Ay + gh[2] * Az + hh4[0] * b.q[0] + hh4[1] * b.q[1] + hh4[2] * b.q[2] + hh4[3] * b.q[3];
      const float dLdv = (dLdw - S) * inv;
      r = dLdv * u * d2 * (2.0f * b.inv2r2);
    }
    float red[13];
#pragma unroll
    for (int e = 0; e < 12; e++) red[e] = wave_sum(w * P[e]);
    red[12] = wave_sum(r);
    if (lane == 63) {
#pragma unroll
      for (int e = 0; e < 13; e++) atomicAdd(&s_acc[k][e], red[e]);
    }
  }
  const float t0 = wave_sum(gh[0]), t1 = wave_sum(gh[1]), t2 = wave_sum(gh[2]);
  if (lane == 63) { atomicAdd(&s_gt[0], t0); atomicAdd(&s_gt[1], t1); atomicAdd(&s_gt[2], t2); }
  __syncthreads();
  for (int e = t; e < B * 13; e += 256) {
    const int k = e / 13, c = e % 13;
    const float v = s_acc[k][c];
    if (c < 12) atomicAdd(&a.dG[12 * (k + 1) + c], v);
    else atomicAdd(&a.drho[k + 1], v);
  }
  if (t < 3) atomicAdd(&a.dgt[t], s_gt[t]);
}

// lbs_backward_bonelane_kernel (all bones) for J > 64.  A lane keeps the 13 sums of at most LBW_PASS blocks of 8 bones in
// registers, so the bones are walked in passes of LBW_PASS blocks.  The per-Gaussian normaliser spans every bone: a first walk
// over the wave's listed Gaussians computes it (and dL/dmotion_mask) and leaves (1/sum, S) in LDS; each gradient pass then
// recomputes its bones' terms.  Same per-workgroup partials and finish kernel as the <= 64-joint form.
#define LBW_NBLK (MAX_J_WIDE / LB_BONES)  // 32 blocks of 8 bones
#define LBW_PASS 8                         // blocks per gradient pass
template <bool MOD>
__global__ __launch_bounds__(256) void lbs_backward_bonelane_wide_kernel(LbsArgs a) {
  constexpr int GPB = LB_GPB;
  __shared__ Bone bones[LBW_NBLK * LB_BONES];
  __shared__ float s_acc[LBW_NBLK * LB_BONES][13];
  __shared__ float s_gt[3];
  __shared__ float2 s_norm[4][GPB / 4];
  __shared__ unsigned short s_list[4][GPB / 4];
  const int B = a.J - 1;
  const int nblk = (B + LB_BONES - 1) / LB_BONES;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane >> 3, bl = lane & 7;
  const int wave_first = blockIdx.x * GPB + wave * (GPB / 4);
  const int wave_end = min(a.N, wave_first + GPB / 4);
  lbs_bonelane_prologue(a, bones, s_acc, s_gt, nblk);
  // the wave's Gaussians with an incoming gradient, listed (the others: zeros of the per-Gaussian outputs)
  int n_work = 0;
#pragma unroll 1
  for (int g = 0; g < GPB / 4 / 64; g++) {
    const int n = wave_first + 64 * g + lane;
    bool touched = false;
    if (n < wave_end) {
      const float4 hq = reinterpret_cast<const float4*>(a.g_rot)[n];
      touched = (a.g_xyz[3 * n] != 0.f) || (a.g_xyz[3 * n + 1] != 0.f) || (a.g_xyz[3 * n + 2] != 0.f) ||
                (hq.x != 0.f) || (hq.y != 0.f) || (hq.z != 0.f) || (hq.w != 0.f);
      if (!touched && a.dmask) a.dmask[n] = 0.f;
      if (!touched && MOD) {
        for (int k = 0; k < B; k++) a.dmod[(size_t)n * B + k] = 0.f;
      }
    }
    const uint64_t tm = __builtin_amdgcn_ballot_w64(touched);
    if (touched) s_list[wave][n_work + __builtin_popcountll(tm & ((1ull << lane) - 1ull))] = (unsigned short)(64 * g + lane);
    n_work += __builtin_popcountll(tm);
  }
  struct StepOps { int n; bool valid; float px, py, pz, m, g0, g1, g2; float4 h; };
  auto fetch = [&](int w0) {
    StepOps o;
    o.valid = w0 + slot < n_work;
    o.n = o.valid ? wave_first + (int)s_list[wave][w0 + slot] : 0;
    o.px = 0.f; o.py = 0.f; o.pz = 0.f; o.m = 0.f; o.g0 = 0.f; o.g1 = 0.f; o.g2 = 0.f;
    o.h = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o.valid) {
      o.px = a.x[3 * o.n]; o.py = a.x[3 * o.n + 1]; o.pz = a.x[3 * o.n + 2];
      o.m = a.motion_mask ? a.motion_mask[o.n] : 1.0f;
      o.g0 = a.g_xyz[3 * o.n]; o.g1 = a.g_xyz[3 * o.n + 1]; o.g2 = a.g_xyz[3 * o.n + 2];
      o.h = reinterpret_cast<const float4*>(a.g_rot)[o.n];
    }
    return o;
  };
  const float gx = a.global_trans[0], gy = a.global_trans[1], gz = a.global_trans[2];
  // the normaliser over every bone: sum_k v_k and S = sum_k w_k dL/dw_k
#pragma unroll 1
  for (int w0 = 0; w0 < n_work; w0 += 8) {
    const StepOps cu = fetch(w0);
    const float px = cu.px, py = cu.py, pz = cu.pz, m = cu.m;
    const float gh0 = cu.g0 * m, gh1 = cu.g1 * m, gh2 = cu.g2 * m;
    const float hh0 = cu.h.x * m, hh1 = cu.h.y * m, hh2 = cu.h.z * m, hh3 = cu.h.w * m;
    float sum = 0.f, sv = 0.f, su = 0.f;
#pragma unroll 2
    for (int bb = 0; bb < nblk; bb++) {
      const int k = bb * LB_BONES + bl;
      const Bone& b = bones[k];
      const float d2 = bone_d2_fast(b, px, py, pz);
      const bool on = cu.valid && (k < B);
      const float u = on ? fast_exp(-d2 * b.inv2r2) : 0.f;
      float v;
      if constexpr (MOD) v = on ? u * a.weight_mod[(size_t)cu.n * B + k] + 1e-7f : 0.f;
      else v = on ? u + 1e-7f : 0.f;
      const float Ax = b.G[0] * px + b.G[1] * py + b.G[2] * pz + b.G[3];
      const float Ay = b.G[4] * px + b.G[5] * py + b.G[6] * pz + b.G[7];
      const float Az = b.G[8] * px + b.G[9] * py + b.G[10] * pz + b.G[11];
      const float dw = gh0 * Ax + gh1 * Ay + gh2 * Az + hh0 * b.q[0] + hh1 * b.q[1] + hh2 * b.q[2] + hh3 * b.q[3];
      const float du = cu.g0 * Ax + cu.g1 * Ay + cu.g2 * Az + cu.h.x * b.q[0] + cu.h.y * b.q[1] + cu.h.z * b.q[2] + cu.h.w * b.q[3];
      sum += v;
      sv += v * dw;
      su += v * du;
    }
    sum = row8_sum(sum);
    sv = row8_sum(sv);
    const float inv = cu.valid ? 1.0f / sum : 0.f;
    const float S = sv * inv;
    if (a.dmask) {
      su = row8_sum(su);
      if (cu.valid && bl == 0) a.dmask[cu.n] = su * inv + cu.g0 * (gx - px) + cu.g1 * (gy - py) + cu.g2 * (gz - pz);
    }
    if (cu.valid && bl == 0) s_norm[wave][w0 + slot] = make_float2(inv, S);
  }
  __syncthreads();
  float gt0 = 0.f, gt1 = 0.f, gt2 = 0.f;
#pragma unroll 1
  for (int p0 = 0; p0 < nblk; p0 += LBW_PASS) {
    float acc[LBW_PASS][13];
#pragma unroll
    for (int bb = 0; bb < LBW_PASS; bb++)
#pragma unroll
      for (int e = 0; e < 13; e++) acc[bb][e] = 0.f;
#pragma unroll 1
    for (int w0 = 0; w0 < n_work; w0 += 8) {
      const StepOps cu = fetch(w0);
      const bool valid = cu.valid;
      const int n = cu.n;
      const float px = cu.px, py = cu.py, pz = cu.pz, m = cu.m;
      const float2 nrm = valid ? s_norm[wave][w0 + slot] : make_float2(0.f, 0.f);
      const float inv = nrm.x, S = nrm.y;
      const float gh0 = cu.g0 * m, gh1 = cu.g1 * m, gh2 = cu.g2 * m;
      const float hh0 = cu.h.x * m, hh1 = cu.h.y * m, hh2 = cu.h.z * m, hh3 = cu.h.w * m;
      const float P[12] = {gh0 * px, gh0 * py, gh0 * pz, gh0, gh1 * px, gh1 * py, gh1 * pz, gh1,
                           gh2 * px, gh2 * py, gh2 * pz, gh2};
#pragma unroll
      for (int bb = 0; bb < LBW_PASS; bb++) {
        if (p0 + bb >= nblk) break;
        const int k = (p0 + bb) * LB_BONES + bl;
        const Bone& b = bones[k];
        const float d2 = bone_d2_fast(b, px, py, pz);
        const bool on = valid && (k < B);
        const float u = on ? fast_exp(-d2 * b.inv2r2) : 0.f;
        float md = 1.0f, v;
        if constexpr (MOD) {
          md = on ? a.weight_mod[(size_t)n * B + k] : 1.0f;
          v = on ? u * md + 1e-7f : 0.f;
        } else {
          v = on ? u + 1e-7f : 0.f;
        }
        const float Ax = b.G[0] * px + b.G[1] * py + b.G[2] * pz + b.G[3];
        const float Ay = b.G[4] * px + b.G[5] * py + b.G[6] * pz + b.G[7];
        const float Az = b.G[8] * px + b.G[9] * py + b.G[10] * pz + b.G[11];
        const float dw = gh0 * Ax + gh1 * Ay + gh2 * Az + hh0 * b.q[0] + hh1 * b.q[1] + hh2 * b.q[2] + hh3 * b.q[3];
        const float w = v * inv;
        const float dLdv = (dw - S) * inv;
        float r;
        if constexpr (MOD) r = dLdv * md * u * d2 * (2.0f * b.inv2r2);
        else r = dLdv * u * d2 * (2.0f * b.inv2r2);
        if (MOD && on) a.dmod[(size_t)n * B + k] = dLdv * u;  // v = u * mod + 1e-7
#pragma unroll
        for (int e = 0; e < 12; e++) acc[bb][e] += w * P[e];
        acc[bb][12] += r;
      }
      if (p0 == 0 && bl == 0) { gt0 += gh0; gt1 += gh1; gt2 += gh2; }
    }
    // fold the 8 slot rows (lanes l, l^8, l^16, l^32) into the workgroup's sums of this pass's bones
#pragma unroll
    for (int bb = 0; bb < LBW_PASS; bb++) {
      if (p0 + bb >= nblk) break;
#pragma unroll
      for (int e = 0; e < 13; e++) {
        float t = acc[bb][e];
        t += __shfl_xor(t, 8); t += __shfl_xor(t, 16); t += __shfl_xor(t, 32);
        if (slot == 0) atomicAdd(&s_acc[(p0 + bb) * LB_BONES + bl][e], t);
      }
    }
  }
  gt0 = wave_sum(gt0); gt1 = wave_sum(gt1); gt2 = wave_sum(gt2);
  if (lane == 63) { atomicAdd(&s_gt[0], gt0); atomicAdd(&s_gt[1], gt1); atomicAdd(&s_gt[2], gt2); }
  __syncthreads();
  float* part = a.partial + (size_t)blockIdx.x * (B * 13 + 3);
  for (int e = threadIdx.x; e < B * 13; e += 256) part[e] = (&s_acc[0][0])[e];
  if (threadIdx.x < 3) part[B * 13 + threadIdx.x] = s_gt[threadIdx.x];
}

// ==================================================================================== playback: a pose track, skin colours
// Inference only (riggs_lbs_sequence_forward, riggs_skinning_colors).  What depends on the canonical cloud alone — a Gaussian's
// position, its top-K selection set, its weight_mod row, the bones' segments and radii — is computed or staged ONCE; the M poses
// of a track then differ in the bones' (G, q) records only.  The distances and the selection are the forward's own functions (Bone,
// bone_geometry, bone_d2 / bone_d2_fast, topk_select, fast_exp).  Three pieces of lbs_forward_kernel / fk_forward_kernel are written
// out again below as helpers that only the playback kernels call — fk_write_out, stage_mod_tile, bone_weight: the forward keeps
// its own lines, because a shared form of such lines has changed the compiled code of kernels on the benchmark's path before
// (the note at the top of this file); they must be kept in step by hand, and tests/test_gpu_playback.py compares the two paths.
struct SeqArgs {
  int M;             // frames of the track
  int slice_frames;  // frames per blockIdx.y: a multiple of the pass F
  int gt_stride;     // floats between two frames' global_trans: 3, or 0 (one translation for the whole track)
};

// what a chain kernel leaves for its joint (a restatement of fk_forward_kernel's write-out)
__device__ __forceinline__ void fk_write_out(int j, const float (&G)[12], const FkIn& in, const float* __restrict__ gt,
                                             float* __restrict__ transforms, float* __restrict__ node_rot, float* __restrict__ d_nodes) {
  const float x = in.x[0], y = in.x[1], z = in.x[2];
#pragma unroll
  for (int e = 0; e < 12; e++) transforms[12 * j + e] = G[e];
#pragma unroll
  for (int r = 0; r < 3; r++) d_nodes[3 * j + r] = (G[4 * r] * x + G[4 * r + 1] * y + G[4 * r + 2] * z + G[4 * r + 3]) + gt[r];
  float q[4];
  R_to_quat(G, q);
#pragma unroll
  for (int e = 0; e < 4; e++) node_rot[4 * j + e] = q[e];
}
// the kinematic chain of every frame of a track: one wave per frame (<= 64 joints) ...
__global__ __launch_bounds__(64) void fk_sequence_kernel(int J, int gt_stride, const float* __restrict__ local_rot,
                                                         const float* __restrict__ joints, const int32_t* __restrict__ parents,
                                                         const float* __restrict__ global_trans, float* __restrict__ transforms,
                                                         float* __restrict__ node_rot, float* __restrict__ d_nodes) {
  const size_t f = blockIdx.x;
  FkIn in;
  fk_load(J, local_rot + f * J * 4, joints, parents, nullptr, nullptr, in);
  FkLane fl;
  fk_wave_forward(J, in, fl);
  const int j = threadIdx.x;
  if (j < J) fk_write_out(j, fl.G, in, global_trans + f * gt_stride, transforms + f * J * 12, node_rot + f * J * 4, d_nodes + f * J * 3);
}
// ... or one 256-thread workgroup per frame (65..256 joints)
__global__ __launch_bounds__(256) void fk_sequence_wide_kernel(int J, int gt_stride, const float* __restrict__ local_rot,
                                                               const float* __restrict__ joints, const int32_t* __restrict__ parents,
                                                               const float* __restrict__ global_trans, float* __restrict__ transforms,
                                                               float* __restrict__ node_rot, float* __restrict__ d_nodes) {
  __shared__ FkWideShared sh;
  const size_t f = blockIdx.x;
  const int j = threadIdx.x;
  FkIn in;
  fk_load_joint(j, J, local_rot + f * J * 4, joints, parents, nullptr, nullptr, in);
  FkWide fw;
  fk_block_forward(J, in, fw, sh);
  if (j < J) {
    float G[12];
#pragma unroll
    for (int e = 0; e < 12; e++) G[e] = sh.G[j][e];
    fk_write_out(j, G, in, global_trans + f * gt_stride, transforms + f * J * 12, node_rot + f * J * 4, d_nodes + f * J * 3);
  }
}

// the bones' pose-independent records (their G / q stay zero: the track's poses have records of their own)
__device__ __forceinline__ void stage_bone_geometry(const LbsArgs& a, Bone* bones) {
  for (int k = threadIdx.x; k < a.J - 1; k += blockDim.x) {
    Bone b;
    bone_geometry(a, k, b);
#pragma unroll
    for (int e = 0; e < 12; e++) b.G[e] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) b.q[e] = 0.f;
    bones[k] = b;
  }
  __syncthreads();
}
// a restatement of lbs_forward_kernel's weight_mod tile: the wave's 64 rows, one contiguous run, copied coalesced into a wave-private LDS tile of
// odd row stride (a.mod_lds: the launch reserved 256 (B | 1) floats); nullptr: the rows are read from global memory
__device__ __forceinline__ float* stage_mod_tile(const LbsArgs& a, float* s_mod_dyn, int& BP) {
  if (!a.mod_lds) return nullptr;
  const int Bm = a.J - 1, lane_ = threadIdx.x & 63;
  BP = Bm | 1;
  float* s_mod = s_mod_dyn + (threadIdx.x >> 6) * 64 * BP;
  const int ng = blockIdx.x * 256 + (threadIdx.x & ~63);
  const int n_el = max(0, min(64, a.N - ng)) * Bm;
  const float* run = a.weight_mod + (size_t)ng * Bm;
  const float invB = 1.0f / (float)Bm;
  for (int e = lane_; e < n_el; e += 64) {
    const int r = (int)(((float)e + 0.5f) * invB);
    s_mod[r * BP + (e - r * Bm)] = run[e];
  }
  return s_mod;
}
// v_k = exp(-d2 / (2 r^2)) [* weight_mod] + 1e-7 of the thread's Gaussian and bone k (skeleton_warp.py:66-71): the forward's line, restated
template <bool TOPK>
__device__ __forceinline__ float bone_weight(const LbsArgs& a, const Bone& b, int k, int B, int row, const float* s_mod, int BP,
                                             float px, float py, float pz) {
  const float d2 = TOPK ? bone_d2(b, px, py, pz) : bone_d2_fast(b, px, py, pz);
  float u = fast_exp(-d2 * b.inv2r2);
  if (a.weight_mod) u *= s_mod ? s_mod[(threadIdx.x & 63) * BP + k] : a.weight_mod[(size_t)row * B + k];
  return u + 1e-7f;
}

// One Gaussian per thread, the track in passes of F frames: per pass the F frames' (G, q) records of every bone are staged in
// LDS (64 B per bone and frame), a bone's weight is evaluated once and accumulated into F sets of 16 sums.  gridDim.y slices
// the track where the Gaussians alone leave the device underfilled (each slice repeats the per-Gaussian prologue).
// a.transforms / a.node_rot: (M, J, 12) / (M, J, 4) of the chain launch in front; a.d_xyz / a.d_rot: (M, N, 3) / (M, N, 4).
template <bool TOPK, int MAXJ, int F>
__global__ __launch_bounds__(256) void lbs_sequence_kernel(LbsArgs a, SeqArgs s) {
  typedef std::conditional_t<(MAXJ > MAX_J) && TOPK, SelLds, SelReg> Sel;
  __shared__ Bone bones[MAXJ - 1];
  __shared__ float4 pose[F][MAXJ - 1][4];  // rows of [R|t] of the bone's child joint, then its node_rot
  extern __shared__ float s_mod_dyn[];
  const int B = a.J - 1, J = a.J;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const bool on = n < a.N;
  const int row = min(n, a.N - 1);
  const float px = a.x[3 * row], py = a.x[3 * row + 1], pz = a.x[3 * row + 2];
  const float m = a.motion_mask ? a.motion_mask[row] : 1.0f;
  int BP = 0;
  const float* s_mod = stage_mod_tile(a, s_mod_dyn, BP);
  stage_bone_geometry(a, bones);
  Sel sel;
  if constexpr (Sel::in_lds) {
    __shared__ typename Sel::Column s_sel;
    sel.col = s_sel;
  }
  if (TOPK) topk_select(sel, bones, B, a.K, px, py, pz);
  const int f_begin = blockIdx.y * s.slice_frames, f_end = min(s.M, f_begin + s.slice_frames);
  for (int f0 = f_begin; f0 < f_end; f0 += F) {
    const int nf = min(F, f_end - f0);
    __syncthreads();  // (the previous pass has read its records)
    for (int e = threadIdx.x; e < F * B; e += 256) {
      const int f = e / B, k = e - f * B;
      float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0, g2 = g0, q = g0;
      if (f < nf) {
        const size_t jf = (size_t)(f0 + f) * J + (k + 1);
        const float4* G = reinterpret_cast<const float4*>(a.transforms + jf * 12);
        g0 = G[0]; g1 = G[1]; g2 = G[2];
        q = *reinterpret_cast<const float4*>(a.node_rot + jf * 4);
      }
      pose[f][k][0] = g0; pose[f][k][1] = g1; pose[f][k][2] = g2; pose[f][k][3] = q;
    }
    __syncthreads();
    float acc[F][16], sum = 0.f;
#pragma unroll
    for (int f = 0; f < F; f++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[f][e] = 0.f;
    for (int k = 0; k < B; k++) {
      if (TOPK && !sel.test(k)) continue;
      const float v = bone_weight<TOPK>(a, bones[k], k, B, row, s_mod, BP, px, py, pz);
      sum += v;
#pragma unroll
      for (int f = 0; f < F; f++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float4 g = pose[f][k][r];
          acc[f][4 * r] += v * g.x; acc[f][4 * r + 1] += v * g.y; acc[f][4 * r + 2] += v * g.z; acc[f][4 * r + 3] += v * g.w;
        }
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int f = 0; f < F; f++) {
      if (!on || f >= nf) continue;
      const float* gt = a.global_trans + (size_t)(f0 + f) * s.gt_stride;
      const float* A = acc[f];
      const float ax = (A[0] * px + A[1] * py + A[2] * pz + A[3]) * inv + gt[0];
      const float ay = (A[4] * px + A[5] * py + A[6] * pz + A[7]) * inv + gt[1];
      const float az = (A[8] * px + A[9] * py + A[10] * pz + A[11]) * inv + gt[2];
      const size_t o = (size_t)(f0 + f) * a.N + n;
      a.d_xyz[3 * o] = (ax - px) * m; a.d_xyz[3 * o + 1] = (ay - py) * m; a.d_xyz[3 * o + 2] = (az - pz) * m;
      reinterpret_cast<float4*>(a.d_rot)[o] = make_float4(A[12] * inv * m, A[13] * inv * m, A[14] * inv * m, A[15] * inv * m);
    }
  }
}

// The skinning weights folded into a colour per Gaussian (visualization.py:118-129), nothing of (N, J-1) written:
// mode 0 "blend"   sum_k w_k colour[k + 1]  (bone k <-> child joint k + 1);
// mode 1 "segment" the colour of the bone of the largest weight, the first such bone on equality — a gathered value, unchanged.
template <bool TOPK, int MAXJ>
__global__ __launch_bounds__(256) void skinning_colors_kernel(LbsArgs a, const float* __restrict__ node_colors, int mode,
                                                              float* __restrict__ out) {
  typedef std::conditional_t<(MAXJ > MAX_J) && TOPK, SelLds, SelReg> Sel;
  __shared__ Bone bones[MAXJ - 1];
  __shared__ float s_col[MAXJ - 1][3];
  extern __shared__ float s_mod_dyn[];
  const int B = a.J - 1;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int row = min(n, a.N - 1);
  const float px = a.x[3 * row], py = a.x[3 * row + 1], pz = a.x[3 * row + 2];
  int BP = 0;
  const float* s_mod = stage_mod_tile(a, s_mod_dyn, BP);
  for (int e = threadIdx.x; e < 3 * B; e += 256) (&s_col[0][0])[e] = node_colors[3 + e];
  stage_bone_geometry(a, bones);
  if (n >= a.N) return;
  Sel sel;
  if constexpr (Sel::in_lds) {
    __shared__ typename Sel::Column s_sel;
    sel.col = s_sel;
  }
  if (TOPK) topk_select(sel, bones, B, a.K, px, py, pz);
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, sum = 0.f, best = -1.0f;
  int bi = 0;
  for (int k = 0; k < B; k++) {
    if (TOPK && !sel.test(k)) continue;
    const float v = bone_weight<TOPK>(a, bones[k], k, B, row, s_mod, BP, px, py, pz);
    sum += v;
    c0 += v * s_col[k][0]; c1 += v * s_col[k][1]; c2 += v * s_col[k][2];
    if (v > best) { best = v; bi = k; }
  }
  if (mode == 1) {
    out[3 * n] = s_col[bi][0]; out[3 * n + 1] = s_col[bi][1]; out[3 * n + 2] = s_col[bi][2];
  } else {
    const float inv = 1.0f / sum;
    out[3 * n] = c0 * inv; out[3 * n + 1] = c1 * inv; out[3 * n + 2] = c2 * inv;
  }
}

}  // namespace riggs

using namespace riggs;

static int fill_lbs(LbsArgs& a, int32_t N, int32_t J, int32_t K, const float* x, const float* joints,
                    const int32_t* parents, const float* rho, const float* transforms, const float* node_rot,
                    const float* gt, const float* mask) {
  RIGGS_REQUIRE(J >= 2 && J <= MAX_J_WIDE, "num_joints must be in [2, 256]");
  RIGGS_REQUIRE(N >= 0, "num_points < 0");
  RIGGS_REQUIRE(K < J, "K must be < num_joints");
  memset(&a, 0, sizeof(a));
  a.N = N; a.J = J; a.K = K; a.x = x; a.joints = joints; a.parents = parents; a.node_radius_log = rho;
  a.transforms = transforms; a.node_rot = node_rot; a.global_trans = gt; a.motion_mask = mask;
  return 0;
}

// two Gaussians per thread in the all-bones forward (see lbs_forward_kernel) where the launch still fills the chip
static bool lbs_two_per_thread(int N, int J) { return N >= LBS_PTS2_MIN_N && J >= LBS_PTS2_MIN_J; }

static unsigned lbs_grid(int N, int pts) { return (unsigned)((N + 256 * pts - 1) / (256 * pts)); }
// The bone records through the scalar cache (lbs_forward_scalar_kernel) where that wins: the large, many-joint scenes whose loop is
// bound by the LDS handing every wave the records (2 M x 64: 129 -> 104 us; at 300 k x 24 the extra one-workgroup launch in front
// costs what the loop gains: 13.0 against 15.9 us — tools/lbs_scalar_ab.py); the caller must have handed over a table
// (riggs_lbs_bone_table_bytes).  riggs_set_option("lbs_scalar", 1) forces it at every size (the A/B), -1 forbids it.
static bool lbs_use_scalar(const LbsArgs& a, const void* bone_table) {
  if (!bone_table || a.K > 0 || a.weight_mod) return false;
  const int o = option(OPT_LBS_SCALAR);
  return o > 0 || (o == 0 && lbs_two_per_thread(a.N, a.J));
}
// the forward's weight_mod tile (one Gaussian per thread, up to 47 bones: 48 KB; beyond, the rows are read from global memory)
static size_t lbs_mod_lds(LbsArgs& a, int pts) {
  a.mod_lds = (a.weight_mod && pts == 1 && a.J - 1 <= 47) ? 1 : 0;
  return a.mod_lds ? (size_t)256 * ((a.J - 1) | 1) * sizeof(float) : 0;
}

// The forward's launches, FK: with the kinematic chain inside (the <= 64-joint forms; beyond, the caller has run it in front).
// Wide, then the scalar table, then LDS: top-K, or two Gaussians per thread, or one per thread with the weight_mod tile.
template <bool FK>
static int launch_lbs_forward(LbsArgs& a, void* bone_table, hipStream_t s) {
  const int N = a.N, J = a.J;
  if (J > MAX_J) {  // (the bone table is a <= 64-joint form)
    ProfScope ps(PROF_LBS_FWD, s);
    if (a.K > 0) hipLaunchKernelGGL((lbs_forward_kernel<true, false, 1, MAX_J_WIDE>), dim3(lbs_grid(N, 1)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((lbs_forward_kernel<false, false, 1, MAX_J_WIDE>), dim3(lbs_grid(N, 1)), dim3(256), 0, s, a);
  } else if (lbs_use_scalar(a, bone_table) && !a.nn_weight && !a.nn_idx) {
    Bone* table = (Bone*)bone_table;
    if constexpr (FK) hipLaunchKernelGGL(lbs_fk_table_kernel, dim3(1), dim3(64), 0, s, a, table);
    else hipLaunchKernelGGL(lbs_bone_table_kernel, dim3(1), dim3(64), 0, s, a, table);
    ProfScope ps(PROF_LBS_FWD, s);
    if (lbs_two_per_thread(N, J)) hipLaunchKernelGGL((lbs_forward_scalar_kernel<2>), dim3(lbs_grid(N, 2)), dim3(256), 0, s, a, table);
    else hipLaunchKernelGGL((lbs_forward_scalar_kernel<1>), dim3(lbs_grid(N, 1)), dim3(256), 0, s, a, table);
  } else {
    ProfScope ps(PROF_LBS_FWD, s);
    a.table_out = (Bone*)bone_table;  // (may be NULL)
    if (a.K > 0) hipLaunchKernelGGL((lbs_forward_kernel<true, FK, 1>), dim3(lbs_grid(N, 1)), dim3(256), 0, s, a);
    else if (lbs_two_per_thread(N, J)) hipLaunchKernelGGL((lbs_forward_kernel<false, FK, 2>), dim3(lbs_grid(N, 2)), dim3(256), 0, s, a);
    else { const size_t lds = lbs_mod_lds(a, 1); hipLaunchKernelGGL((lbs_forward_kernel<false, FK, 1>), dim3(lbs_grid(N, 1)), dim3(256), lds, s, a); }
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" {

int riggs_fk_forward(int32_t J, const float* local_rot, const float* joints, const int32_t* parents,
                     const float* global_trans, float* transforms, float* node_rot, float* d_nodes,
                     riggs_stream stream) {
  RIGGS_REQUIRE(J >= 1 && J <= MAX_J_WIDE, "num_joints must be in [1, 256]");
  {
    ProfScope ps(PROF_FK_FWD, (hipStream_t)stream);
    if (J <= MAX_J) hipLaunchKernelGGL(fk_forward_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, J, local_rot, joints, parents,
                                       global_trans, transforms, node_rot, d_nodes);
    else hipLaunchKernelGGL(fk_forward_wide_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, J, local_rot, joints, parents,
                            global_trans, transforms, node_rot, d_nodes);
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_fk_backward(int32_t J, const float* local_rot, const float* joints, const int32_t* parents,
                      const float* dL_dtransforms, const float* dL_dd_nodes, float* dL_dlocal_rot,
                      float* dL_dglobal_trans, riggs_stream stream) {
  RIGGS_REQUIRE(J >= 1 && J <= MAX_J_WIDE, "num_joints must be in [1, 256]");
  {
    ProfScope ps(PROF_FK_BWD, (hipStream_t)stream);
    if (J <= MAX_J) hipLaunchKernelGGL(fk_backward_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, J, local_rot, joints, parents,
                                       dL_dtransforms, dL_dd_nodes, dL_dlocal_rot, dL_dglobal_trans);
    else hipLaunchKernelGGL(fk_backward_wide_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, J, local_rot, joints, parents,
                            dL_dtransforms, dL_dd_nodes, dL_dlocal_rot, dL_dglobal_trans);
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_lbs_forward(int32_t N, int32_t J, int32_t K, const float* x, const float* joints, const int32_t* parents,
                      const float* node_radius_log, const float* transforms, const float* node_rot,
                      const float* global_trans, const float* motion_mask, const float* weight_mod, float* d_xyz,
                      float* d_rotation, float* nn_weight, int64_t* nn_idx, void* bone_table, riggs_stream stream) {
  LbsArgs a;
  int rc = fill_lbs(a, N, J, K, x, joints, parents, node_radius_log, transforms, node_rot, global_trans, motion_mask);
  if (rc) return rc;
  a.d_xyz = d_xyz; a.d_rot = d_rotation; a.nn_weight = nn_weight; a.nn_idx = nn_idx;
  a.weight_mod = weight_mod;
  RIGGS_REQUIRE(weight_mod == nullptr || K <= 0, "weight_mod is supported with K = -1 (all bones) only");
  if (N == 0) return 0;
  return launch_lbs_forward<false>(a, bone_table, (hipStream_t)stream);
}

int riggs_lbs_forward_fk(int32_t N, int32_t J, int32_t K, const float* x, const float* joints, const int32_t* parents,
                         const float* node_radius_log, const float* local_rot, const float* global_trans,
                         const float* motion_mask, const float* weight_mod, float* transforms, float* node_rot, float* d_nodes,
                         float* d_xyz, float* d_rotation, void* bone_table, riggs_stream stream) {
  LbsArgs a;
  int rc = fill_lbs(a, N, J, K, x, joints, parents, node_radius_log, transforms, node_rot, global_trans, motion_mask);
  if (rc) return rc;
  a.d_xyz = d_xyz; a.d_rot = d_rotation;
  a.weight_mod = weight_mod;
  a.local_rot = local_rot; a.fk_transforms = transforms; a.fk_node_rot = node_rot; a.fk_d_nodes = d_nodes;
  RIGGS_REQUIRE(weight_mod == nullptr || K <= 0, "weight_mod is supported with K = -1 (all bones) only");
  RIGGS_REQUIRE(local_rot && transforms && node_rot && d_nodes, "riggs_lbs_forward_fk needs the pose and the three chain outputs");
  if (N == 0) return riggs_fk_forward(J, local_rot, joints, parents, global_trans, transforms, node_rot, d_nodes, stream);
  if (J > MAX_J) {
    // the wide chain as a launch of its own in front of the skinning: inside every workgroup it would cost each of them the
    // whole sweep (one barrier per level: a 256-joint chain is 255 levels)
    rc = riggs_fk_forward(J, local_rot, joints, parents, global_trans, transforms, node_rot, d_nodes, stream);
    if (rc) return rc;
  }
  return launch_lbs_forward<true>(a, bone_table, (hipStream_t)stream);
}

size_t riggs_lbs_bone_table_bytes(void) { return sizeof(Bone) * MAX_J; }

size_t riggs_lbs_backward_workspace_bytes(int32_t N, int32_t J) {
  const size_t blocks = (size_t)(N > 0 ? (N + LB_GPB - 1) / LB_GPB : 1);
  return align_up(blocks * ((size_t)(J - 1) * 13 + 3) * sizeof(float));
}

int riggs_lbs_backward(int32_t N, int32_t J, int32_t K, const float* x, const float* joints, const int32_t* parents,
                       const float* node_radius_log, const float* transforms, const float* node_rot,
                       const float* global_trans, const float* motion_mask, const float* weight_mod,
                       const float* g_xyz, const float* g_rot, float* dL_dtransforms, float* dL_dnode_radius_log,
                       float* dL_dglobal_trans, float* dL_dmotion_mask, float* dL_dweight_mod, void* workspace,
                       riggs_stream stream) {
  return riggs_lbs_backward_table(N, J, K, x, joints, parents, node_radius_log, transforms, node_rot, global_trans, motion_mask,
                                  weight_mod, g_xyz, g_rot, dL_dtransforms, dL_dnode_radius_log, dL_dglobal_trans, dL_dmotion_mask,
                                  dL_dweight_mod, nullptr, workspace, stream);
}

int riggs_lbs_backward_table(int32_t N, int32_t J, int32_t K, const float* x, const float* joints, const int32_t* parents,
                             const float* node_radius_log, const float* transforms, const float* node_rot,
                             const float* global_trans, const float* motion_mask, const float* weight_mod,
                             const float* g_xyz, const float* g_rot, float* dL_dtransforms, float* dL_dnode_radius_log,
                             float* dL_dglobal_trans, float* dL_dmotion_mask, float* dL_dweight_mod, const void* bone_table,
                             void* workspace, riggs_stream stream) {
  LbsArgs a;
  int rc = fill_lbs(a, N, J, K, x, joints, parents, node_radius_log, transforms, node_rot, global_trans, motion_mask);
  if (rc) return rc;
  a.g_xyz = g_xyz; a.g_rot = g_rot; a.dG = dL_dtransforms; a.drho = dL_dnode_radius_log; a.dgt = dL_dglobal_trans;
  a.dmask = dL_dmotion_mask;
  a.weight_mod = weight_mod; a.dmod = dL_dweight_mod;
  a.table_in = J <= MAX_J ? (const Bone*)bone_table : nullptr;  // (skeletons of more joints never wrote one)
  RIGGS_REQUIRE(weight_mod == nullptr || (K <= 0 && dL_dweight_mod != nullptr), "weight_mod needs K = -1 and dL_dweight_mod");
  a.partial = (float*)workspace;
  RIGGS_REQUIRE(workspace != nullptr, "riggs_lbs_backward needs its workspace");
  hipStream_t s = (hipStream_t)stream;
  if (N == 0 || K > 0) {  // the top-K (thread-per-Gaussian) path accumulates into zeroed outputs
    RIGGS_HIP_CHECK(hipMemsetAsync(dL_dtransforms, 0, (size_t)J * 48, s));
    RIGGS_HIP_CHECK(hipMemsetAsync(dL_dnode_radius_log, 0, (size_t)J * 4, s));
    RIGGS_HIP_CHECK(hipMemsetAsync(dL_dglobal_trans, 0, 12, s));
  }
  if (N == 0) return 0;
  {
    ProfScope ps(PROF_LBS_BWD, s);
    const int nblk = (J - 1 + LB_BONES - 1) / LB_BONES;
    if (J > MAX_J) {
      if (K > 0) hipLaunchKernelGGL(lbs_backward_wide_kernel, dim3((N + 255) / 256), dim3(256), 0, s, a);
      else {
        const int blocks = (N + LB_GPB - 1) / LB_GPB;
        if (a.weight_mod) hipLaunchKernelGGL(lbs_backward_bonelane_wide_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(lbs_backward_bonelane_wide_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
        hipLaunchKernelGGL(lbs_backward_finish_kernel, dim3((J - 1) * 13 + 3), dim3(256), 0, s, a, blocks);
      }
    } else if (K > 0) hipLaunchKernelGGL(lbs_backward_kernel, dim3((N + 255) / 256), dim3(256), 0, s, a);
    else switch (nblk) {
      case 1: launch_lbs_bwd_bonelane<1>(a, s); break;
      case 2: launch_lbs_bwd_bonelane<2>(a, s); break;
      case 3: launch_lbs_bwd_bonelane<3>(a, s); break;
      case 4: launch_lbs_bwd_bonelane<4>(a, s); break;
      case 5: launch_lbs_bwd_bonelane<5>(a, s); break;
      case 6: launch_lbs_bwd_bonelane<6>(a, s); break;
      case 7: launch_lbs_bwd_bonelane<7>(a, s); break;
      default: launch_lbs_bwd_bonelane<8>(a, s); break;
    }
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"

// ---- playback: the launches
// Frames per pass, by joint range.  A workgroup's static LDS stays within 64 KB: the bones' records (112 B each), F pose records
// per bone (64 B each) and, for the top-K form beyond 64 joints, the 8 KB of selection columns —
//   <= 64 joints  F = 4:  7.1 + 16.1 KB        (F = 4: the weight — ~20 vector instructions and an exp — is then a fifth of a
//   <= 128 joints F = 4: 14.2 + 32.5 (+ 8) KB   bone's 64 multiply-adds, and 64 sums leave the kernel four waves per SIMD)
//   <= 256 joints F = 2: 28.6 + 32.6 KB; top-K F = 1: 28.6 + 16.3 + 8 KB
static int seq_pass_frames(int J, int K) { return J <= 128 ? 4 : (K > 0 ? 1 : 2); }
template <bool TOPK, int MAXJ, int F>
static constexpr size_t seq_static_lds() {
  return sizeof(Bone) * (MAXJ - 1) + sizeof(float4) * 4 * F * (MAXJ - 1) + ((MAXJ > MAX_J && TOPK) ? sizeof(SelLds::Column) : 0);
}
static_assert(seq_static_lds<true, MAX_J, 4>() <= 65536 && seq_static_lds<true, 128, 4>() <= 65536 &&
              seq_static_lds<false, MAX_J_WIDE, 2>() <= 65536 && seq_static_lds<true, MAX_J_WIDE, 1>() <= 65536, "64 KB of static LDS");
// the weight_mod tile (256 (B | 1) floats, dynamic) where it fits beside `static_bytes` in 64 KB
static size_t seq_mod_lds(LbsArgs& a, size_t static_bytes) {
  const size_t tile = (size_t)256 * ((a.J - 1) | 1) * sizeof(float);
  a.mod_lds = (a.weight_mod && static_bytes + tile <= 65536) ? 1 : 0;
  return a.mod_lds ? tile : 0;
}
template <bool TOPK, int MAXJ, int F>
static void launch_lbs_sequence(LbsArgs& a, const SeqArgs& s, dim3 grid, hipStream_t st) {
  const size_t lds = seq_mod_lds(a, seq_static_lds<TOPK, MAXJ, F>());
  hipLaunchKernelGGL((lbs_sequence_kernel<TOPK, MAXJ, F>), grid, dim3(256), lds, st, a, s);
}
template <bool TOPK, int MAXJ>
static void launch_skinning_colors(LbsArgs& a, const float* node_colors, int mode, float* out, hipStream_t st) {
  const size_t fixed = sizeof(Bone) * (MAXJ - 1) + 12 * (MAXJ - 1) + ((MAXJ > MAX_J && TOPK) ? sizeof(SelLds::Column) : 0);
  const size_t lds = seq_mod_lds(a, fixed);
  hipLaunchKernelGGL((skinning_colors_kernel<TOPK, MAXJ>), dim3(lbs_grid(a.N, 1)), dim3(256), lds, st, a, node_colors, mode, out);
}

// the current device's compute units, asked once per device ordinal (two runtime calls off the per-chunk path)
static int seq_compute_units(int& cus) {
  static int cached[64];  // 0: not asked yet
  int dev = 0;
  RIGGS_HIP_CHECK(hipGetDevice(&dev));
  int& c = cached[dev & 63];
  if (c <= 0) RIGGS_HIP_CHECK(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev));
  cus = c;
  return 0;
}

extern "C" {

int32_t riggs_lbs_sequence_pass_frames(int32_t J, int32_t K) { return seq_pass_frames(J, K); }

int riggs_lbs_sequence_forward(int32_t N, int32_t M, int32_t J, int32_t K, const float* x, const float* joints, const int32_t* parents,
                               const float* node_radius_log, const float* local_rot, const float* global_trans,
                               int32_t global_trans_stride, const float* motion_mask, const float* weight_mod, float* transforms,
                               float* node_rot, float* d_nodes, float* d_xyz, float* d_rotation, riggs_stream stream) {
  LbsArgs a;
  int rc = fill_lbs(a, N, J, K, x, joints, parents, node_radius_log, transforms, node_rot, global_trans, motion_mask);
  if (rc) return rc;
  RIGGS_REQUIRE(M >= 0, "num_frames < 0");
  RIGGS_REQUIRE(global_trans_stride == 0 || global_trans_stride == 3, "global_trans_stride must be 3 (per frame) or 0 (one for the track)");
  RIGGS_REQUIRE(weight_mod == nullptr || K <= 0, "weight_mod is supported with K = -1 (all bones) only");
  RIGGS_REQUIRE(local_rot && transforms && node_rot && d_nodes, "riggs_lbs_sequence_forward needs the poses and the three chain outputs");
  a.d_xyz = d_xyz; a.d_rot = d_rotation; a.weight_mod = weight_mod;
  if (M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (J <= MAX_J) hipLaunchKernelGGL(fk_sequence_kernel, dim3(M), dim3(64), 0, st, J, global_trans_stride, local_rot, joints, parents,
                                     global_trans, transforms, node_rot, d_nodes);
  else hipLaunchKernelGGL(fk_sequence_wide_kernel, dim3(M), dim3(256), 0, st, J, global_trans_stride, local_rot, joints, parents,
                          global_trans, transforms, node_rot, d_nodes);
  RIGGS_HIP_CHECK(hipGetLastError());
  if (N == 0) return 0;
  // The grid: ceil(N / 256) workgroups walk the whole track each.  Where that is fewer than two workgroups per compute unit
  // (eight waves: two per SIMD, the least that overlaps one wave's LDS reads with another's arithmetic), the track's passes are
  // dealt over gridDim.y until it is — each slice pays the per-Gaussian prologue again, so no further.
  const int F = seq_pass_frames(J, K);
  const int passes = (M + F - 1) / F, blocks_x = (int)lbs_grid(N, 1);
  int cus = 0;
  if (seq_compute_units(cus)) return 1;
  int slices = (2 * cus + blocks_x - 1) / blocks_x;
  if (slices < 1) slices = 1;
  if (slices > passes) slices = passes;
  const int slice_passes = (passes + slices - 1) / slices;
  SeqArgs s;
  s.M = M; s.slice_frames = slice_passes * F; s.gt_stride = global_trans_stride;
  const dim3 grid(blocks_x, (passes + slice_passes - 1) / slice_passes);
  // (not under a ProfScope: the profiler's skinning slot is the per-frame forward's)
  if (J <= MAX_J) {
    if (K > 0) launch_lbs_sequence<true, MAX_J, 4>(a, s, grid, st); else launch_lbs_sequence<false, MAX_J, 4>(a, s, grid, st);
  } else if (J <= 128) {
    if (K > 0) launch_lbs_sequence<true, 128, 4>(a, s, grid, st); else launch_lbs_sequence<false, 128, 4>(a, s, grid, st);
  } else {
    if (K > 0) launch_lbs_sequence<true, MAX_J_WIDE, 1>(a, s, grid, st); else launch_lbs_sequence<false, MAX_J_WIDE, 2>(a, s, grid, st);
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

int riggs_skinning_colors(int32_t N, int32_t J, int32_t K, const float* x, const float* joints, const int32_t* parents,
                          const float* node_radius_log, const float* weight_mod, const float* node_colors, int32_t mode,
                          float* colors, riggs_stream stream) {
  LbsArgs a;
  int rc = fill_lbs(a, N, J, K, x, joints, parents, node_radius_log, nullptr, nullptr, nullptr, nullptr);
  if (rc) return rc;
  RIGGS_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (blend) or 1 (segment)");
  RIGGS_REQUIRE(weight_mod == nullptr || K <= 0, "weight_mod is supported with K = -1 (all bones) only");
  RIGGS_REQUIRE(node_colors && colors, "riggs_skinning_colors needs the node colours and the output");
  a.weight_mod = weight_mod;
  if (N == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (J <= MAX_J) {
    if (K > 0) launch_skinning_colors<true, MAX_J>(a, node_colors, mode, colors, st); else launch_skinning_colors<false, MAX_J>(a, node_colors, mode, colors, st);
  } else {
    if (K > 0) launch_skinning_colors<true, MAX_J_WIDE>(a, node_colors, mode, colors, st); else launch_skinning_colors<false, MAX_J_WIDE>(a, node_colors, mode, colors, st);
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
