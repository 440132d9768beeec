// The frame of a pose solver, once: what ik.hip (riggs_ik_solve) and fit.hip (riggs_fit_pose) do around their own solve for the step
// (ik.hip: a 3E x 3E dual system by Cholesky; fit.hip: matrix-free PCG over tree sweeps).  ONE workgroup per problem b = blockIdx.x,
// thread j owns joint j; J <= 64 on one wave64 (fk_wave_*), 65 .. 256 on 256 threads through LDS (fk_block_*): SolveChain<WIDE>.
//   inputs   a parent outside [0, j) is clamped into it (the walks end, no index leaves the arrays); q from local_rot_in[b]; locked;
//            global_trans_in[b]; damping and max_step times the extent under the bits of `relative`                    solve_load
//   chain    topology and the first sweep once, the level sweep per iteration; posed_j = G_j [x_j; 1] + global_trans      forward, sweep, posed
//   step     r = s (target - posed), the difference shortened to max_step first (Buss & Kim 2005, section 3)              clamped_step
//   turn     "step 5": delta_a = R(G_vp(a))^T omega_a (the root: omega_0), theta = |delta_a|; theta > 0:
//            q_a <- (cos theta/2, sin(theta/2) delta_a / theta) (x) q_a; global_trans += its step                         turn
//   result   local_rot_out, d_nodes, global_trans_out; the residual |target - posed| (who has none: each solver's rule)   solve_write, solve_distance
// Both files are built with -ffp-contract=off and -fno-fast-math: a helper that keeps an expression's tree keeps its bits
// (tools/pose_solve_bits.py; profiles/pose_solve_bits.json).  Included by ik.hip, fit.hip and bones.hip (a third solver: its operators) only.
#pragma once
#include "fk_device.h"

#include <type_traits>

namespace riggs {

// ---- the level sweep alone, for a caller that changes the rotations and runs the chain again (ik.hip: once per iteration).
// `f` (and `sh`) come from an earlier fk_wave_forward / fk_block_forward over the same parents, whose topology — levels,
// children, the deepest level — is kept; the local transforms are renewed from in.q and the sweep G_i = G_parent(i) T_i is the
// forward's, operation for operation.  Call with all lanes (threads) of the wave (workgroup).
__device__ __forceinline__ void fk_wave_sweep(int J, const FkIn& in, FkLane& f) {
  const int j = threadIdx.x & 63;
  if (j < J) fk_local_T(in, f.T);
#pragma unroll
  for (int e = 0; e < 12; e++) f.G[e] = f.T[e];
  for (int l = 1; l <= f.maxlev; l++) {
    float Gp[12];
#pragma unroll
    for (int e = 0; e < 12; e++) Gp[e] = fk_lane_get(f.G[e], f.par);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) {
        float v = Gp[4 * r] * f.T[c] + Gp[4 * r + 1] * f.T[4 + c] + Gp[4 * r + 2] * f.T[8 + c];
        if (c == 3) v += Gp[4 * r + 3];
        if (j >= 1) f.G[4 * r + c] = v;
      }
  }
}

// ... over the block: sh.G is rewritten (behind a barrier: the previous sweep's readers are done) and final behind the last one.
__device__ __forceinline__ void fk_block_sweep(int J, const FkIn& in, FkWide& f, FkWideShared& sh) {
  const int j = threadIdx.x;
  const bool on = j < J;
  if (on) fk_local_T(in, f.T);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 12; e++) sh.G[j][e] = f.T[e];
  __syncthreads();
  for (int l = 1; l <= f.maxlev; l++) {
    if (on && f.lev == l) {
      float Gp[12];
#pragma unroll
      for (int e = 0; e < 12; e++) Gp[e] = sh.G[f.par][e];
      float G[12];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
          float v = Gp[4 * r] * f.T[c] + Gp[4 * r + 1] * f.T[4 + c] + Gp[4 * r + 2] * f.T[8 + c];
          if (c == 3) v += Gp[4 * r + 3];
          G[4 * r + c] = v;
        }
#pragma unroll
      for (int e = 0; e < 12; e++) sh.G[j][e] = G[e];
    }
    __syncthreads();
  }
}

// ---- sums over the tree, for a caller whose operator is a sum along root-to-joint paths and its transpose a sum over subtrees
// (fit.hip: the Jacobian of the chain and its transpose).  They run on the topology an earlier fk_wave_forward / fk_block_forward
// left in `f` (`sh`): the same levels, the same children, the same order.  Call with all lanes (threads) of the wave (workgroup).
// fk_*_prefix:  v_j <- v_vp(j) + v_j level by level from the root: v_j becomes the sum over the path root .. j.
// fk_*_subtree: v_a <- v_a + the finished sums of a's children in descending child index, deepest level first (the order of the
// sequential sweep i = J - 1 .. 1 and of fk_*_backward): v_a becomes the sum over a's subtree, a included.
template <int N>
__device__ __forceinline__ void fk_wave_prefix(const FkLane& f, float (&v)[N]) {
  for (int l = 1; l <= f.maxlev; l++) {
#pragma unroll
    for (int e = 0; e < N; e++) {
      const float t = fk_lane_get(v[e], f.par);
      if (f.lev == l) v[e] = t + v[e];
    }
  }
}
template <int N>
__device__ __forceinline__ void fk_wave_subtree(int J, const FkLane& f, float (&v)[N]) {
  const int j = threadIdx.x & 63;
  for (int l = f.maxlev - 1; l >= 0; l--) {
    unsigned long long km = (j < J && f.lev == l) ? f.kids : 0ull;
    while (__builtin_amdgcn_ballot_w64(km != 0ull) != 0ull) {
      const bool has = km != 0ull;
      const int i = has ? 63 - __builtin_clzll(km) : j;  // descending child index
#pragma unroll
      for (int e = 0; e < N; e++) {
        const float t = fk_lane_get(v[e], i);
        if (has) v[e] += t;
      }
      if (has) km &= ~(1ull << i);
    }
  }
}
// ... over the block, through `buf` (MAX_J_WIDE rows of at least N floats in LDS): ONE barrier per level.  The first write of a
// call lands behind the last read of the call before it only if a barrier lies between the two calls: the caller's business
// (fit.hip: a dot product's reduction, or the other sweep, always does).  fk_block_prefix leaves every row of `buf` final behind
// its last barrier; rows >= J hold what their threads passed in.
template <int N, int S>
__device__ __forceinline__ void fk_block_prefix(int J, const FkWide& f, float (*buf)[S], float (&v)[N]) {
  static_assert(N <= S, "fk_block_prefix: the row is too short");
  const int j = threadIdx.x;
#pragma unroll
  for (int e = 0; e < N; e++) buf[j][e] = v[e];
  __syncthreads();
  for (int l = 1; l <= f.maxlev; l++) {
    if (j < J && f.lev == l) {
#pragma unroll
      for (int e = 0; e < N; e++) { v[e] = buf[f.par][e] + v[e]; buf[j][e] = v[e]; }
    }
    __syncthreads();
  }
}
template <int N, int S>
__device__ __forceinline__ void fk_block_subtree(int J, const FkWide& f, const FkWideShared& sh, float (*buf)[S], float (&v)[N]) {
  static_assert(N <= S, "fk_block_subtree: the row is too short");
  const int j = threadIdx.x;
  const bool on = j < J;
  for (int l = f.maxlev - 1; l >= 0; l--) {
    if (on && f.lev == l + 1) {
#pragma unroll
      for (int e = 0; e < N; e++) buf[j][e] = v[e];
    }
    __syncthreads();
    if (on && f.lev == l) {
      for (int w = FK_WIDE_WORDS - 1; w >= 0; w--) {
        uint32_t km = sh.kids[j][w];
        while (km != 0u) {
          const int b = 31 - __builtin_clz(km);  // descending child index
          const int i = 32 * w + b;
#pragma unroll
          for (int e = 0; e < N; e++) v[e] += buf[i][e];
          km &= ~(1u << b);
        }
      }
    }
  }
}

// ---- what the two entries' arguments have in common (IkArgs / FitArgs hold one, plus their own)
struct SolveArgs {
  int J, iterations, relative, solve_translation;
  float damping, max_step;
  const float* joints; const int32_t* parents; const float* local_rot_in; const float* global_trans_in;
  const uint8_t* locked; const float* extent;
  float* local_rot_out; float* global_trans_out; float* d_nodes; float* residual;
};

// (host) the checks the two entries share, under the entry's `name`, and the SolveArgs -> 0, or 2 with the error set.  What differs
// stays with the entries: ik.hip needs `extent` only under a bit of `relative`, fit.hip always.
inline int solve_args(const char* name, int32_t B, int32_t J, const float* joints, const int32_t* parents, const float* local_rot_in,
                      const float* global_trans_in, const uint8_t* locked, int32_t iterations, float damping, float max_step,
                      const float* extent, int32_t relative, int32_t solve_translation, float* local_rot_out, float* global_trans_out,
                      float* d_nodes, float* residual, SolveArgs& a) {
#define SOLVE_REQUIRE(cond, text) if (!(cond)) { set_error("%s: %s (%s:%d)", name, text, __FILE__, __LINE__); return 2; }
  SOLVE_REQUIRE(B >= 1, "needs B >= 1");
  SOLVE_REQUIRE(J >= 1 && J <= MAX_J_WIDE, "num_joints must be in [1, 256]");
  SOLVE_REQUIRE(iterations >= 0, "iterations >= 0");
  SOLVE_REQUIRE((relative & ~3) == 0, "relative is a mask of bits 0 and 1");
  SOLVE_REQUIRE(damping > 0.f && max_step >= 0.f, "needs damping > 0 and max_step >= 0");  // (a NaN fails both)
  SOLVE_REQUIRE(joints && parents && local_rot_in && global_trans_in && local_rot_out && global_trans_out && d_nodes && residual, "NULL argument");
#undef SOLVE_REQUIRE
  a = {J, iterations, relative, solve_translation != 0, damping, max_step, joints, parents, local_rot_in, global_trans_in,
       locked, extent, local_rot_out, global_trans_out, d_nodes, residual};
  return 0;
}

// ---- the problem as thread j holds it
struct SolveIn {
  FkIn in;                          // the thread's joint; in.q is what the iterations turn
  bool locked;
  float damping2, max_step;         // the scaled constants: the same values in every thread
};
// `ext`: the rig's extent as the caller reads it (ik.hip: 1 where `extent` is NULL).  `gt`, global_trans (every thread the same
// values), is an array of the caller's own: solve_write indexes it by the thread, which a member of `p` would pay for in scratch.
__device__ __forceinline__ void solve_load(const SolveArgs& a, int b, int j, float ext, SolveIn& p, float (&gt)[3]) {
  p.in = {};
  p.in.q[0] = 1.f;
  p.locked = false;
  if (j < a.J) {
    int vp = 0;
    if (j >= 1) vp = min(max(a.parents[j], 0), j - 1);
    p.in.par = vp;
#pragma unroll
    for (int e = 0; e < 4; e++) p.in.q[e] = a.local_rot_in[((size_t)b * a.J + j) * 4 + e];
#pragma unroll
    for (int e = 0; e < 3; e++) { p.in.x[e] = a.joints[3 * j + e]; p.in.c[e] = a.joints[3 * vp + e]; }
    p.locked = a.locked && a.locked[j] != 0;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) gt[c] = a.global_trans_in[(size_t)b * 3 + c];
  const float damping = (a.relative & 1) ? a.damping * ext : a.damping;
  p.max_step = (a.relative & 2) ? a.max_step * ext : a.max_step;
  p.damping2 = damping * damping;
}

__device__ __forceinline__ void clamped_step(const float (&target)[3], const float (&posed)[3], float max_step, float s, float (&r)[3]) {
  float d[3];
#pragma unroll
  for (int c = 0; c < 3; c++) d[c] = target[c] - posed[c];
  const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (len > max_step) {
    const float k = max_step / len;
#pragma unroll
    for (int c = 0; c < 3; c++) d[c] = d[c] * k;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) r[c] = s * d[c];
}

__device__ __forceinline__ float solve_distance(const float (&target)[3], const float (&posed)[3]) {
  const float d0 = target[0] - posed[0], d1 = target[1] - posed[1], d2 = target[2] - posed[2];
  return sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
}

// `pos`: the posed skeleton of the final quaternions in LDS, behind a barrier.  The residual is the caller's.
__device__ __forceinline__ void solve_write(const SolveArgs& a, int b, int j, const SolveIn& p, const float (&gt)[3], const float (*pos)[3]) {
  if (j < a.J) {
#pragma unroll
    for (int e = 0; e < 4; e++) a.local_rot_out[((size_t)b * a.J + j) * 4 + e] = p.in.q[e];
#pragma unroll
    for (int c = 0; c < 3; c++) a.d_nodes[((size_t)b * a.J + j) * 3 + c] = pos[j][c];
  }
  if (j < 3) a.global_trans_out[(size_t)b * 3 + j] = gt[j];
}

// ---- the chain in its two forms.  `sh` is the block form's LDS (one wave keeps everything in registers: an empty struct, no
// LDS).  Every function is called by all threads of the workgroup: the block form has barriers inside, the wave form lane shuffles.
// `f` is a local of the kernel's own, handed to every function.  The tree sums (fk_*_prefix / fk_*_subtree above) are NOT wrapped
// here: fit.hip calls them in their two forms itself, because through a wrapper of this struct the same lines cost
// fit_pose_kernel<false> 11 VGPRs and 13 % of its time (NOTES.md "Pose solvers: one frame").
struct SolveNoLds {};
template <bool WIDE>
struct SolveChain {
  typedef typename std::conditional<WIDE, FkWideShared, SolveNoLds>::type Shared;
  typedef typename std::conditional<WIDE, FkWide, FkLane>::type Fk;

  static __device__ __forceinline__ void forward(int J, const FkIn& in, Fk& f, Shared& sh) {  // the topology and the first sweep
    if constexpr (WIDE) fk_block_forward(J, in, f, sh); else fk_wave_forward(J, in, f);
  }
  static __device__ __forceinline__ void sweep(int J, const FkIn& in, Fk& f, Shared& sh) {  // a later one, from the in.q of now
    if constexpr (WIDE) fk_block_sweep(J, in, f, sh); else fk_wave_sweep(J, in, f);
  }
  // element e of the thread's own G, and of joint i's (one wave: by lane shuffle, taken by every lane)
  static __device__ __forceinline__ float own_G(const Fk& f, const Shared& sh, int e) { if constexpr (WIDE) return sh.G[threadIdx.x][e]; else return f.G[e]; }
  static __device__ __forceinline__ float G_of(const Fk& f, const Shared& sh, int i, int e) { if constexpr (WIDE) return sh.G[i][e]; else return fk_lane_get(f.G[e], i); }
  // posed_j as fk_forward_kernel forms d_nodes, operation for operation, into the caller's LDS row (`on`: j < J)
  static __device__ __forceinline__ void posed(const Fk& f, const Shared& sh, const SolveIn& p, const float (&gt)[3], bool on, float (&pos)[3]) {
    float G[12];
#pragma unroll
    for (int e = 0; e < 12; e++) G[e] = own_G(f, sh, e);
    if (on) {
#pragma unroll
      for (int r = 0; r < 3; r++) pos[r] = (G[4 * r] * p.in.x[0] + G[4 * r + 1] * p.in.x[1] + G[4 * r + 2] * p.in.x[2] + G[4 * r + 3]) + gt[r];
    }
  }
  // step 5 for the thread's joint: the world-frame rotation vector `om` into the parent's frame and onto p.in.q where `turns`
  // (the solver's guard) and theta > 0; with `trans`, global_trans += dgt
  static __device__ __forceinline__ void turn(const Fk& f, const Shared& sh, const float (&om)[3], bool turns, bool trans, const float (&dgt)[3],
                                              SolveIn& p, float (&gt)[3]) {
    float Rp[9], dl[3];  // the parent's rotation
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) Rp[3 * r + c] = G_of(f, sh, p.in.par, 4 * r + c);
#pragma unroll
    for (int c = 0; c < 3; c++) dl[c] = (threadIdx.x == 0) ? om[c] : Rp[c] * om[0] + Rp[3 + c] * om[1] + Rp[6 + c] * om[2];
    const float th = sqrtf(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
    if (turns && th > 0.f) {
      const float half = 0.5f * th, k = sinf(half) / th;
      const float aw = cosf(half), ax = k * dl[0], ay = k * dl[1], az = k * dl[2];
      const float bw = p.in.q[0], bx = p.in.q[1], by = p.in.q[2], bz = p.in.q[3];
      p.in.q[0] = aw * bw - ax * bx - ay * by - az * bz;
      p.in.q[1] = aw * bx + ax * bw + ay * bz - az * by;
      p.in.q[2] = aw * by - ax * bz + ay * bw + az * bx;
      p.in.q[3] = aw * bz + ax * by - ay * bx + az * bw;
    }
    if (trans) {
#pragma unroll
      for (int c = 0; c < 3; c++) gt[c] = gt[c] + dgt[c];
    }
  }
};

}  // namespace riggs
