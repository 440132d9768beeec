// Whole-skeleton pose fitting (riggs_amd/pose_edit.py: fit_pose): every joint may have a target position, and the rig's pose is
// turned so that the posed joints reach them.  Levenberg-Marquardt (Levenberg 1944, Marquardt 1963: damped Gauss-Newton) with the
// clamped target step of Buss & Kim (2005, section 3) on the rig's own kinematics; the damped normal equations are solved
// matrix-free by a fixed number of Jacobi-preconditioned conjugate-gradient steps (Hestenes & Stiefel 1952).  Restated from the
// published methods; the reference has nothing like it.  tests/fit_ref.py is the NumPy restatement this kernel is held to.
//
// Kinematics as in ik.hip: joint a turns about piv_a = posed_vp(a), the root about itself; a's subtree includes a.  Unknowns: one
// world-frame rotation vector omega_a per unlocked joint and, with solve_translation, tau' = tau / extent.  Positions enter the
// operators relative to the posed ROOT, pc_j = posed_j - posed_0 (J and J^T do not change under a common shift: the shift's
// terms cancel along every path); this keeps every cancelling difference below within one rig extent of its operands, wherever
// global_trans has put the rig.  One iteration:
//   1  FK (fk_forward_kernel's arithmetic); s_h = sqrt(w_h) for live targets (w_h > 0), else 0 and the target is never read;
//      r_h = s_h clamp(target_h - posed_h, max_step)
//   2  down (J p):   W_j = W_vp(j) + omega_j, C_j = C_vp(j) + omega_j x piv_j;  u_h = s_h ((W_h x pc_h - C_h) + extent tau')
//      up (J^T u):   F_a = sum_subtree s_h u_h, M_a = sum_subtree pc_h x (s_h u_h);  g_a = M_a - piv_a x F_a (locked: 0),
//                    g_tau' = extent F_0;   A = J^T J + lambda^2 I
//   3  preconditioner from the subtree moments about the posed root, S0 = sum s^2, S1 = sum s^2 pc, S2 = sum s^2 |pc|^2:
//      d_a = max((S2 - 2 piv_a . S1) + |piv_a|^2 S0, 0),  Minv_a = 1 / (2/3 d_a + lambda^2),  Minv_tau' = 1 / (extent^2 S0_0 + lambda^2)
//      (one up-sweep of 11 values together with b = J^T r)
//   4  cg_steps steps of PCG from x = 0 on A x = b; before a step: stop unless r.z > FIT_CG_EPS * (r.z at the start); stop
//      unless p.Ap > 0.  The updates behind the last step's x are not computed.
//   5  IK's step 5 with omega_a = x_a; global_trans += extent x_tau'
// and one more FK behind the last iteration for d_nodes and the residual.  The inputs, the FK and the clamped step of 1, 5 and the
// result are the frame this solver shares with ik.hip: pose_solve.h has them, here are the operators, 3 and 4.
//
// ONE workgroup per problem, ALL iterations in one launch; thread j owns joint j and keeps q, x, r, p, z and Minv in registers;
// every thread carries the three tau' components (the same values).  J <= 64: one wave64, the sweeps by lane shuffles
// (fk_wave_prefix / fk_wave_subtree); 65 .. 256: 256 threads, the sweeps through LDS with one barrier per level (fk_block_*).
// The topology is computed once (fk_*_forward).  A parent adds its children in descending child index.  A dot product: every
// thread forms (a0 b0 + a1 b1) + a2 b2, a wave adds its 64 with wave_sum (a balanced binary tree over adjacent lanes), lane 63
// leaves the sum in LDS together with what the root has to tell everyone (F_0, S0_0), one barrier, every thread adds the waves in
// wave order and the tau' term last: one LDS round trip, two slots in turn.  No float atomics: the same inputs give the same
// bits, and a problem never reads its neighbours.  What bounds it is the chain of dependent steps (levels x 2 sweeps x cg_steps
// x iterations), not bytes.
#include "pose_solve.h"

namespace riggs {

#define FIT_CG_EPS 1e-10f  // (include/riggs_hip.h states it; tests/fit_ref.py: CG_EPS)

struct FitArgs {
  SolveArgs s;
  int cg_steps;
  const float* targets; const float* weights;
};

template <bool WIDE>
struct FitShared {  // (one wave sweeps and sums by lane shuffles: it touches none of this, and no LDS is set aside for it)
  typename SolveChain<WIDE>::Shared fk;  // fk.A is the up-sweeps' row buffer
  float dn[WIDE ? MAX_J_WIDE : 1][8];    // the down-sweeps' row buffer
  float part[2][8];                      // a dot product's slot: the four waves' sums, then the root's four values
};

__device__ __forceinline__ float dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// The workgroup's sum of `term`, the same bits in every thread; root[0..3] of thread 0 reaches every thread on the same trip.
template <bool WIDE>
__device__ __forceinline__ float fit_dot(float term, float (&root)[4], FitShared<WIDE>& ws, int& slot) {
  if constexpr (WIDE) {
    const int j = threadIdx.x;
    const float v = wave_sum(term);
    if ((j & (RIGGS_WAVE - 1)) == RIGGS_WAVE - 1) ws.part[slot][j / RIGGS_WAVE] = v;
    if (j == 0) {
#pragma unroll
      for (int e = 0; e < 4; e++) ws.part[slot][4 + e] = root[e];
    }
    __syncthreads();
    const float sum = ((ws.part[slot][0] + ws.part[slot][1]) + ws.part[slot][2]) + ws.part[slot][3];
#pragma unroll
    for (int e = 0; e < 4; e++) root[e] = ws.part[slot][4 + e];
    slot ^= 1;  // (the slot is written again two calls on: every thread has passed the next call's barrier, behind its reads here)
    return sum;
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) root[e] = fk_lane_get(root[e], 0);
    return wave_sum_bcast(term);
  }
}

template <bool WIDE>
__global__ __launch_bounds__(WIDE ? 256 : 64) void fit_pose_kernel(FitArgs a) {
  constexpr int NJ = WIDE ? MAX_J_WIDE : MAX_J;
  __shared__ float pos[NJ][3];  // posed joints of this iteration
  __shared__ FitShared<WIDE> wsh;
  const int b = blockIdx.x, j = threadIdx.x;
  const int J = a.s.J;
  const bool on = j < J;

  // ---- the problem's inputs (pose_solve.h), then the joint's target
  const float ext = a.s.extent[0];
  SolveIn pr;
  float gt[3];
  solve_load(a.s, b, j, ext, pr, gt);
  bool live = false;
  float s = 0.f, tg[3] = {0.f, 0.f, 0.f};
  if (on) {
    const float w = a.weights ? a.weights[(size_t)b * J + j] : 1.f;
    live = w > 0.f;  // (a NaN weight: off)
    if (live) {      // a target without weight is not read at all
      s = sqrtf(w);
#pragma unroll
      for (int c = 0; c < 3; c++) tg[c] = a.targets[((size_t)b * J + j) * 3 + c];
    }
  }
  const bool turn = on && !pr.locked;
  const float damping2 = pr.damping2;
  const bool trans = a.s.solve_translation != 0;
  int slot = 0;

  // ---- topology and the first sweep
  typedef SolveChain<WIDE> Chain;
  typename Chain::Fk f;
  Chain::forward(J, pr.in, f, wsh.fk);

  for (int it = 0;; it++) {
    if (it > 0) Chain::sweep(J, pr.in, f, wsh.fk);
    Chain::posed(f, wsh.fk, pr, gt, on, pos[j]);
    __syncthreads();
    if (it >= a.s.iterations) break;

    // ---- 1: positions about the posed root, the clamped weighted step
    float pc[3] = {0.f, 0.f, 0.f}, pv[3] = {0.f, 0.f, 0.f}, rr[3] = {0.f, 0.f, 0.f};
    if (on) {
#pragma unroll
      for (int c = 0; c < 3; c++) { pc[c] = pos[j][c] - pos[0][c]; pv[c] = pos[pr.in.par][c] - pos[0][c]; }
    }
    if (live) clamped_step(tg, pos[j], pr.max_step, s, rr);
    // ---- 3 (and b = J^T r): one up-sweep of F, M, S0, S1, S2
    float bq[3], minv;
    float root[4];
    {
      float v[11], fh[3], mh[3];
#pragma unroll
      for (int c = 0; c < 3; c++) fh[c] = s * rr[c];
      cross3(pc, fh, mh);
      const float s2 = s * s;
#pragma unroll
      for (int c = 0; c < 3; c++) { v[c] = fh[c]; v[3 + c] = mh[c]; v[7 + c] = s2 * pc[c]; }
      v[6] = s2;
      v[10] = s2 * dot3(pc, pc);
      if constexpr (WIDE) fk_block_subtree(J, f, wsh.fk, wsh.fk.A, v);  // (written out in both forms, here and twice below:
      else fk_wave_subtree(J, f, v);                                    // through a wrapper this kernel is 13 % slower, pose_solve.h)
      const float F[3] = {v[0], v[1], v[2]}, S1[3] = {v[7], v[8], v[9]};
      float pf[3];
      cross3(pv, F, pf);
#pragma unroll
      for (int c = 0; c < 3; c++) bq[c] = turn ? v[3 + c] - pf[c] : 0.f;
      const float dd = fmaxf((v[10] - 2.f * dot3(pv, S1)) + dot3(pv, pv) * v[6], 0.f);
      minv = 1.f / ((2.f / 3.f) * dd + damping2);
      root[0] = v[0]; root[1] = v[1]; root[2] = v[2]; root[3] = v[6];
    }
    // ---- 4: PCG from x = 0
    float x[3] = {0.f, 0.f, 0.f}, r[3], z[3], p[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { r[c] = bq[c]; z[c] = minv * r[c]; p[c] = z[c]; }
    float rz = fit_dot(dot3(r, z), root, wsh, slot);
    float xt[3] = {0.f, 0.f, 0.f}, rt[3] = {0.f, 0.f, 0.f}, zt[3] = {0.f, 0.f, 0.f}, pt[3] = {0.f, 0.f, 0.f}, minvt = 0.f;
    if (trans) {
      minvt = 1.f / ((ext * ext) * root[3] + damping2);
#pragma unroll
      for (int c = 0; c < 3; c++) { rt[c] = ext * root[c]; zt[c] = minvt * rt[c]; pt[c] = zt[c]; }
      rz = rz + dot3(rt, zt);
    }
    const float rz0 = rz;
    for (int k = 0; k < a.cg_steps; k++) {
      if (!(rz > FIT_CG_EPS * rz0)) break;  // (uniform: every thread holds the same rz)
      // down: W, C along the paths
      float u[3];
      {
        float v[6], c0[3];
        cross3(p, pv, c0);
#pragma unroll
        for (int c = 0; c < 3; c++) { v[c] = p[c]; v[3 + c] = c0[c]; }
        if constexpr (WIDE) fk_block_prefix(J, f, wsh.dn, v);
        else fk_wave_prefix(f, v);
        const float W[3] = {v[0], v[1], v[2]};
        float wp[3];
        cross3(W, pc, wp);
#pragma unroll
        for (int c = 0; c < 3; c++) u[c] = s * ((wp[c] - v[3 + c]) + (trans ? ext * pt[c] : 0.f));
      }
      // up: F, M over the subtrees
      float Ap[3], Apt[3] = {0.f, 0.f, 0.f};
      {
        float v[6], fh[3], mh[3];
#pragma unroll
        for (int c = 0; c < 3; c++) fh[c] = s * u[c];
        cross3(pc, fh, mh);
#pragma unroll
        for (int c = 0; c < 3; c++) { v[c] = fh[c]; v[3 + c] = mh[c]; }
        if constexpr (WIDE) fk_block_subtree(J, f, wsh.fk, wsh.fk.A, v);
        else fk_wave_subtree(J, f, v);
        const float F[3] = {v[0], v[1], v[2]};
        float pf[3];
        cross3(pv, F, pf);
#pragma unroll
        for (int c = 0; c < 3; c++) Ap[c] = turn ? (v[3 + c] - pf[c]) + damping2 * p[c] : 0.f;
        root[0] = v[0]; root[1] = v[1]; root[2] = v[2]; root[3] = 0.f;
      }
      float pAp = fit_dot(dot3(p, Ap), root, wsh, slot);
      if (trans) {
#pragma unroll
        for (int c = 0; c < 3; c++) Apt[c] = ext * root[c] + damping2 * pt[c];
        pAp = pAp + dot3(pt, Apt);
      }
      if (!(pAp > 0.f)) break;
      const float alpha = rz / pAp;
#pragma unroll
      for (int c = 0; c < 3; c++) { x[c] = x[c] + alpha * p[c]; xt[c] = xt[c] + alpha * pt[c]; }
      if (k + 1 == a.cg_steps) break;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        r[c] = r[c] - alpha * Ap[c]; z[c] = minv * r[c];
        rt[c] = rt[c] - alpha * Apt[c]; zt[c] = minvt * rt[c];
      }
      const float rzn = fit_dot(dot3(r, z), root, wsh, slot) + dot3(rt, zt);
      const float beta = rzn / rz;
#pragma unroll
      for (int c = 0; c < 3; c++) { p[c] = z[c] + beta * p[c]; pt[c] = zt[c] + beta * pt[c]; }
      rz = rzn;
    }
    // ---- 5: omega_a = x_a into the parent's frame, onto the quaternion
    const float dgt[3] = {ext * xt[0], ext * xt[1], ext * xt[2]};
    Chain::turn(f, wsh.fk, x, turn, trans, dgt, pr, gt);
  }

  // ---- the result (pos is the posed skeleton of the final quaternions, behind a barrier); a joint without weight: 0
  solve_write(a.s, b, j, pr, gt, pos);
  if (on) a.s.residual[(size_t)b * J + j] = live ? solve_distance(tg, pos[j]) : 0.f;
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_fit_pose(int32_t B, int32_t J, const float* joints, const int32_t* parents, const float* local_rot_in,
                   const float* global_trans_in, const float* targets, const float* weights, const uint8_t* locked,
                   int32_t iterations, int32_t cg_steps, float damping, float max_step, const float* extent, int32_t relative,
                   int32_t solve_translation, float* local_rot_out, float* global_trans_out, float* d_nodes, float* residual,
                   riggs_stream stream) {
  FitArgs a;
  if (int rc = solve_args("riggs_fit_pose", B, J, joints, parents, local_rot_in, global_trans_in, locked, iterations, damping, max_step,
                          extent, relative, solve_translation, local_rot_out, global_trans_out, d_nodes, residual, a.s)) return rc;
  RIGGS_REQUIRE(cg_steps >= 1, "riggs_fit_pose: cg_steps >= 1");
  RIGGS_REQUIRE(targets && extent, "riggs_fit_pose: NULL argument (extent is always needed: it scales the translation unknown)");
  a.cg_steps = cg_steps; a.targets = targets; a.weights = weights;
  if (J <= MAX_J) hipLaunchKernelGGL(fit_pose_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(fit_pose_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
