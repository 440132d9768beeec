// Bone-direction fitting (riggs_amd/pose_edit.py: fit_bones, retarget): every bone h >= 1 (joint h and its parent) may have a target
// DIRECTION, and the rig's pose is turned so that the posed bones point along them.  A direction does not depend on the length of
// the bone it was taken from, so the targets may come from a skeleton of other proportions: a motion-capture clip, another rig's
// track, a rest skeleton extracted anew.  The method is fit.hip's — Levenberg-Marquardt (Levenberg 1944, Marquardt 1963) with the
// clamped target step of Buss & Kim (2005, section 3), the damped normal equations solved matrix-free by a fixed number of
// Jacobi-preconditioned conjugate-gradient steps (Hestenes & Stiefel 1952) — on the UNIT bone vectors instead of the joint
// positions.  Restated from the published methods; the reference has nothing like it.  tests/bones_ref.py is the NumPy restatement
// this kernel is held to.
//
// Kinematics as in fit.hip: joint a turns about posed_vp(a), the root about itself; a's subtree includes a.  Unknowns: one
// world-frame rotation vector omega_a per unlocked joint.  The rig is rigid: a bone only turns, by the sum W_h of the omegas along
// the path root .. h, so its derivative is W_h x beta_h — no pivot enters, the sweeps carry 3 values where fit.hip's carry 6, and the
// translation drops out (global_trans_in is copied to global_trans_out).
// Per problem, once: L_h = |x_h - x_vp(h)|; the target vector v_h is read only if weights[h] > 0 and L_h > 0 (h >= 1);
//   t_h = v_h / |v_h|; the target is live iff also |v_h| > 0 (a NaN fails the comparison: off); s_h = sqrt(w_h) for live h, else 0;
//   S0_a = sum_subtree s^2 does not change with the pose: one up-sweep in front of the loop, Minv_a = 1 / (2/3 S0_a + lambda^2)
//   (|d| = 1: the diagonal block of J^T J is sum s^2 (I - d d^T), whose mean eigenvalue is 2/3 S0).
// One iteration:
//   1  FK (fk_forward_kernel's arithmetic); beta_h = posed_h - posed_vp(h), d_h = beta_h / |beta_h| (live h, else 0);
//      r_h = s_h clamp(t_h - d_h, max_step)
//   2  down (J p):   W_j = W_vp(j) + p_j;  u_h = s_h (W_h x d_h)
//      up (J^T u):   g_a = sum_subtree d_h x (s_h u_h) (locked: 0);   A = J^T J + lambda^2 I,  b = J^T r
//   3  cg_steps steps of PCG from x = 0 on A x = b; before a step: stop unless r.z > BONES_CG_EPS * (r.z at the start); stop
//      unless p.Ap > 0.  The updates behind the last step's x are not computed.
//   4  IK's step 5 with omega_a = x_a
// and one more FK behind the last iteration for d_nodes and the residual |t_h - d_h| (the chord of two unit vectors, in [0, 2];
// 0 where the target is not live).  lambda (damping) and max_step are absolute: directions are dimensionless.  The twist about a
// bone is not observed; CG from x = 0 leaves it where it was.  The inputs, the FK, the clamped step, step 4 and the result are the
// frame of pose_solve.h; here are the operators and the solve.
//
// ONE workgroup per problem, ALL iterations in one launch; thread j owns joint j and keeps q, t, d, x, r, p, z and Minv in
// registers.  J <= 64: one wave64, the sweeps by lane shuffles (fk_wave_prefix / fk_wave_subtree); 65 .. 256: 256 threads, the
// sweeps through LDS with one barrier per level (fk_block_*).  The topology is computed once.  A parent adds its children in
// descending child index.  A dot product is fit.hip's: (a0 b0 + a1 b1) + a2 b2 per thread, wave_sum over each 64, lane 63 leaves
// the sum in LDS, one barrier, every thread adds the four in wave order; two slots in turn.  No float atomics: the same inputs give
// the same bits, and a problem never reads its neighbours.
#include "pose_solve.h"

namespace riggs {

#define BONES_CG_EPS 1e-10f  // (fit.hip's FIT_CG_EPS; include/riggs_hip.h states it; tests/bones_ref.py: CG_EPS)

struct BonesArgs {
  SolveArgs s;
  int cg_steps;
  const float* directions; const float* weights;
};

template <bool WIDE>
struct BonesShared {  // (one wave sweeps and sums by lane shuffles: it touches none of this, and no LDS is set aside for it)
  typename SolveChain<WIDE>::Shared fk;  // fk.A is the up-sweeps' row buffer
  float dn[WIDE ? MAX_J_WIDE : 1][4];    // the down-sweeps' row buffer
  float part[2][4];                      // a dot product's slot: the four waves' sums
};

__device__ __forceinline__ float bones_dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void bones_cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// |v| and v / |v| where `ok` and |v| > 0 (else 0, and false): the ONE form for targets and posed bones, so that a target taken
// from the posed bones is met bit for bit, and a target scaled by a power of two gives the same bits.
__device__ __forceinline__ bool bones_unit(const float (&v)[3], bool ok, float (&u)[3]) {
  const float n = sqrtf(bones_dot3(v, v));
  ok = ok && n > 0.f;  // (a NaN: off)
#pragma unroll
  for (int c = 0; c < 3; c++) u[c] = ok ? v[c] / n : 0.f;
  return ok;
}

// The workgroup's sum of `term`, the same bits in every thread (fit_dot's shape without the root's four values).
template <bool WIDE>
__device__ __forceinline__ float bones_dot(float term, BonesShared<WIDE>& ws, int& slot) {
  if constexpr (WIDE) {
    const int j = threadIdx.x;
    const float v = wave_sum(term);
    if ((j & (RIGGS_WAVE - 1)) == RIGGS_WAVE - 1) ws.part[slot][j / RIGGS_WAVE] = v;
    __syncthreads();
    const float sum = ((ws.part[slot][0] + ws.part[slot][1]) + ws.part[slot][2]) + ws.part[slot][3];
    slot ^= 1;  // (the slot is written again two calls on: every thread has passed the next call's barrier, behind its reads here)
    return sum;
  } else {
    return wave_sum_bcast(term);
  }
}

template <bool WIDE>
__global__ __launch_bounds__(WIDE ? 256 : 64) void fit_bones_kernel(BonesArgs a) {
  constexpr int NJ = WIDE ? MAX_J_WIDE : MAX_J;
  __shared__ float pos[NJ][3];  // posed joints of this iteration
  __shared__ BonesShared<WIDE> wsh;
  const int b = blockIdx.x, j = threadIdx.x;
  const int J = a.s.J;
  const bool on = j < J;

  // ---- the problem's inputs (pose_solve.h), then the bone's target
  SolveIn pr;
  float gt[3];
  solve_load(a.s, b, j, 1.f, pr, gt);
  bool live = false;
  float s = 0.f, tg[3] = {0.f, 0.f, 0.f};
  if (on && j >= 1) {  // (the root has no bone)
    const float w = a.weights ? a.weights[(size_t)b * J + j] : 1.f;
    const float rest[3] = {pr.in.x[0] - pr.in.c[0], pr.in.x[1] - pr.in.c[1], pr.in.x[2] - pr.in.c[2]};
    if (w > 0.f && sqrtf(bones_dot3(rest, rest)) > 0.f) {  // (a NaN weight: off)  a target without weight or bone is not read at all
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; c++) v[c] = a.directions[((size_t)b * J + j) * 3 + c];
      live = bones_unit(v, true, tg);
      if (live) s = sqrtf(w);
    }
  }
  const bool turn = on && !pr.locked;
  const float damping2 = pr.damping2;
  const float zero3[3] = {0.f, 0.f, 0.f};
  int slot = 0;

  // ---- topology and the first sweep; the preconditioner
  typedef SolveChain<WIDE> Chain;
  typename Chain::Fk f;
  Chain::forward(J, pr.in, f, wsh.fk);
  float minv;
  {
    float v[1] = {s * s};
    if constexpr (WIDE) fk_block_subtree(J, f, wsh.fk, wsh.fk.A, v);  // (the tree sums are written out in both forms, as in fit.hip:
    else fk_wave_subtree(J, f, v);                                    // pose_solve.h says what a wrapper costs)
    minv = 1.f / ((2.f / 3.f) * v[0] + damping2);
  }

  float d[3] = {0.f, 0.f, 0.f};
  for (int it = 0;; it++) {
    if (it > 0) Chain::sweep(J, pr.in, f, wsh.fk);
    Chain::posed(f, wsh.fk, pr, gt, on, pos[j]);
    __syncthreads();
    // ---- 1: the posed bone's direction
    {
      float beta[3] = {0.f, 0.f, 0.f};
      if (on) {
#pragma unroll
        for (int c = 0; c < 3; c++) beta[c] = pos[j][c] - pos[pr.in.par][c];
      }
      bones_unit(beta, live, d);
    }
    if (it >= a.s.iterations) break;
    float rr[3] = {0.f, 0.f, 0.f};
    if (live) clamped_step(tg, d, pr.max_step, s, rr);
    // ---- b = J^T r
    float bq[3];
    {
      float v[3], fh[3];
#pragma unroll
      for (int c = 0; c < 3; c++) fh[c] = s * rr[c];
      bones_cross3(d, fh, v);
      if constexpr (WIDE) fk_block_subtree(J, f, wsh.fk, wsh.fk.A, v);
      else fk_wave_subtree(J, f, v);
#pragma unroll
      for (int c = 0; c < 3; c++) bq[c] = turn ? v[c] : 0.f;
    }
    // ---- 3: PCG from x = 0
    float x[3] = {0.f, 0.f, 0.f}, r[3], z[3], p[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { r[c] = bq[c]; z[c] = minv * r[c]; p[c] = z[c]; }
    float rz = bones_dot(bones_dot3(r, z), wsh, slot);
    const float rz0 = rz;
    for (int k = 0; k < a.cg_steps; k++) {
      if (!(rz > BONES_CG_EPS * rz0)) break;  // (uniform: every thread holds the same rz)
      // down: W along the paths
      float u[3];
      {
        float v[3] = {p[0], p[1], p[2]}, wd[3];
        if constexpr (WIDE) fk_block_prefix(J, f, wsh.dn, v);
        else fk_wave_prefix(f, v);
        bones_cross3(v, d, wd);
#pragma unroll
        for (int c = 0; c < 3; c++) u[c] = s * wd[c];
      }
      // up: the moments over the subtrees
      float Ap[3];
      {
        float v[3], fh[3];
#pragma unroll
        for (int c = 0; c < 3; c++) fh[c] = s * u[c];
        bones_cross3(d, fh, v);
        if constexpr (WIDE) fk_block_subtree(J, f, wsh.fk, wsh.fk.A, v);
        else fk_wave_subtree(J, f, v);
#pragma unroll
        for (int c = 0; c < 3; c++) Ap[c] = turn ? v[c] + damping2 * p[c] : 0.f;
      }
      const float pAp = bones_dot(bones_dot3(p, Ap), wsh, slot);
      if (!(pAp > 0.f)) break;
      const float alpha = rz / pAp;
#pragma unroll
      for (int c = 0; c < 3; c++) x[c] = x[c] + alpha * p[c];
      if (k + 1 == a.cg_steps) break;
#pragma unroll
      for (int c = 0; c < 3; c++) { r[c] = r[c] - alpha * Ap[c]; z[c] = minv * r[c]; }
      const float rzn = bones_dot(bones_dot3(r, z), wsh, slot);
      const float beta = rzn / rz;
#pragma unroll
      for (int c = 0; c < 3; c++) p[c] = z[c] + beta * p[c];
      rz = rzn;
    }
    // ---- 4: omega_a = x_a into the parent's frame, onto the quaternion
    Chain::turn(f, wsh.fk, x, turn, false, zero3, pr, gt);
  }

  // ---- the result (pos is the posed skeleton of the final quaternions, behind a barrier); a bone without live target: 0
  solve_write(a.s, b, j, pr, gt, pos);
  if (on) a.s.residual[(size_t)b * J + j] = live ? solve_distance(tg, d) : 0.f;
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_fit_bones(int32_t B, int32_t J, const float* joints, const int32_t* parents, const float* local_rot_in,
                    const float* global_trans_in, const float* directions, const float* weights, const uint8_t* locked,
                    int32_t iterations, int32_t cg_steps, float damping, float max_step, float* local_rot_out,
                    float* global_trans_out, float* d_nodes, float* residual, riggs_stream stream) {
  BonesArgs a;
  if (int rc = solve_args("riggs_fit_bones", B, J, joints, parents, local_rot_in, global_trans_in, locked, iterations, damping, max_step,
                          nullptr, 0, 0, local_rot_out, global_trans_out, d_nodes, residual, a.s)) return rc;
  RIGGS_REQUIRE(cg_steps >= 1, "riggs_fit_bones: cg_steps >= 1");
  RIGGS_REQUIRE(directions, "riggs_fit_bones: NULL argument");
  a.cg_steps = cg_steps; a.directions = directions; a.weights = weights;
  if (J <= MAX_J) hipLaunchKernelGGL(fit_bones_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(fit_bones_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
