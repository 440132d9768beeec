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
// and one more FK behind the last iteration for d_nodes and the residual.
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
#include "fk_device.h"

#include <type_traits>

namespace riggs {

#define FIT_CG_EPS 1e-10f  // (include/riggs_hip.h states it; tests/fit_ref.py: CG_EPS)

struct FitArgs {
  int J, iterations, cg_steps, relative, solve_translation;
  float damping, max_step;
  const float* joints; const int32_t* parents; const float* local_rot_in; const float* global_trans_in;
  const float* targets; const float* weights; const uint8_t* locked; const float* extent;
  float* local_rot_out; float* global_trans_out; float* d_nodes; float* residual;
};

struct FitWideShared {
  FkWideShared fk;              // fk.A is the up-sweeps' row buffer
  float dn[MAX_J_WIDE][8];      // the down-sweeps' row buffer
  float part[2][8];             // a dot product's slot: the four waves' sums, then the root's four values
};

__device__ __forceinline__ float dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// The workgroup's sum of `term`, the same bits in every thread; root[0..3] of thread 0 reaches every thread on the same trip.
template <bool WIDE, typename WS>
__device__ __forceinline__ float fit_dot(float term, float (&root)[4], WS& ws, int& slot) {
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
  __shared__ typename std::conditional<WIDE, FitWideShared, int>::type wsh;
  typedef typename std::conditional<WIDE, FkWide, FkLane>::type Fk;
  const int b = blockIdx.x, j = threadIdx.x;
  const int J = a.J;
  const bool on = j < J;

  // ---- the problem's inputs.  A parent outside [0, j) is clamped into it: no index leaves the arrays.
  FkIn in = {};
  in.q[0] = 1.f;
  bool locked = false, live = false;
  float s = 0.f, tg[3] = {0.f, 0.f, 0.f};
  if (on) {
    int vp = 0;
    if (j >= 1) vp = min(max(a.parents[j], 0), j - 1);
    in.par = vp;
#pragma unroll
    for (int e = 0; e < 4; e++) in.q[e] = a.local_rot_in[((size_t)b * J + j) * 4 + e];
#pragma unroll
    for (int e = 0; e < 3; e++) { in.x[e] = a.joints[3 * j + e]; in.c[e] = a.joints[3 * vp + e]; }
    locked = a.locked && a.locked[j] != 0;
    const float w = a.weights ? a.weights[(size_t)b * J + j] : 1.f;
    live = w > 0.f;  // (a NaN weight: off)
    if (live) {      // a target without weight is not read at all
      s = sqrtf(w);
#pragma unroll
      for (int c = 0; c < 3; c++) tg[c] = a.targets[((size_t)b * J + j) * 3 + c];
    }
  }
  const bool turn = on && !locked;
  float gt[3];
#pragma unroll
  for (int c = 0; c < 3; c++) gt[c] = a.global_trans_in[(size_t)b * 3 + c];
  const float ext = a.extent[0];
  const float damping = (a.relative & 1) ? a.damping * ext : a.damping;
  const float max_step = (a.relative & 2) ? a.max_step * ext : a.max_step;
  const float damping2 = damping * damping;
  const bool trans = a.solve_translation != 0;
  int slot = 0;

  // ---- topology and the first sweep
  Fk f;
  if constexpr (WIDE) fk_block_forward(J, in, f, wsh.fk);
  else fk_wave_forward(J, in, f);

  for (int it = 0;; it++) {
    if (it > 0) {
      if constexpr (WIDE) fk_block_sweep(J, in, f, wsh.fk);
      else fk_wave_sweep(J, in, f);
    }
    float G[12];
#pragma unroll
    for (int e = 0; e < 12; e++) {
      if constexpr (WIDE) G[e] = wsh.fk.G[j][e];
      else G[e] = f.G[e];
    }
    if (on) {
#pragma unroll
      for (int r = 0; r < 3; r++)  // (fk_forward_kernel's d_nodes, operation for operation)
        pos[j][r] = (G[4 * r] * in.x[0] + G[4 * r + 1] * in.x[1] + G[4 * r + 2] * in.x[2] + G[4 * r + 3]) + gt[r];
    }
    __syncthreads();
    if (it >= a.iterations) break;

    // ---- 1: positions about the posed root, the clamped weighted step
    float pc[3] = {0.f, 0.f, 0.f}, pv[3] = {0.f, 0.f, 0.f}, rr[3] = {0.f, 0.f, 0.f};
    if (on) {
#pragma unroll
      for (int c = 0; c < 3; c++) { pc[c] = pos[j][c] - pos[0][c]; pv[c] = pos[in.par][c] - pos[0][c]; }
    }
    if (live) {
      float d[3];
#pragma unroll
      for (int c = 0; c < 3; c++) d[c] = tg[c] - pos[j][c];
      const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      if (len > max_step) {
        const float k = max_step / len;
#pragma unroll
        for (int c = 0; c < 3; c++) d[c] = d[c] * k;
      }
#pragma unroll
      for (int c = 0; c < 3; c++) rr[c] = s * d[c];
    }
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
      if constexpr (WIDE) fk_block_subtree(J, f, wsh.fk, wsh.fk.A, v);
      else fk_wave_subtree(J, f, v);
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
    float rz = fit_dot<WIDE>(dot3(r, z), root, wsh, slot);
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
      float pAp = fit_dot<WIDE>(dot3(p, Ap), root, wsh, slot);
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
      const float rzn = fit_dot<WIDE>(dot3(r, z), root, wsh, slot) + dot3(rt, zt);
      const float beta = rzn / rz;
#pragma unroll
      for (int c = 0; c < 3; c++) { p[c] = z[c] + beta * p[c]; pt[c] = zt[c] + beta * pt[c]; }
      rz = rzn;
    }
    // ---- 5: omega_a = x_a into the parent's frame, onto the quaternion
    float Rp[9];  // the parent's rotation (the lane shuffles are taken by every lane)
#pragma unroll
    for (int r9 = 0; r9 < 3; r9++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if constexpr (WIDE) Rp[3 * r9 + c] = wsh.fk.G[in.par][4 * r9 + c];
        else Rp[3 * r9 + c] = fk_lane_get(f.G[4 * r9 + c], in.par);
      }
    float dl[3];
#pragma unroll
    for (int c = 0; c < 3; c++) dl[c] = (j == 0) ? x[c] : Rp[c] * x[0] + Rp[3 + c] * x[1] + Rp[6 + c] * x[2];
    const float th = sqrtf(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
    if (turn && th > 0.f) {
      const float half = 0.5f * th, k = sinf(half) / th;
      const float aw = cosf(half), ax = k * dl[0], ay = k * dl[1], az = k * dl[2];
      const float bw = in.q[0], bx = in.q[1], by = in.q[2], bz = in.q[3];
      in.q[0] = aw * bw - ax * bx - ay * by - az * bz;
      in.q[1] = aw * bx + ax * bw + ay * bz - az * by;
      in.q[2] = aw * by - ax * bz + ay * bw + az * bx;
      in.q[3] = aw * bz + ax * by - ay * bx + az * bw;
    }
    if (trans) {
#pragma unroll
      for (int c = 0; c < 3; c++) gt[c] = gt[c] + ext * xt[c];
    }
  }

  // ---- the result (pos is the posed skeleton of the final quaternions, behind a barrier)
  if (on) {
#pragma unroll
    for (int e = 0; e < 4; e++) a.local_rot_out[((size_t)b * J + j) * 4 + e] = in.q[e];
#pragma unroll
    for (int c = 0; c < 3; c++) a.d_nodes[((size_t)b * J + j) * 3 + c] = pos[j][c];
    float res = 0.f;
    if (live) {
      const float d0 = tg[0] - pos[j][0], d1 = tg[1] - pos[j][1], d2 = tg[2] - pos[j][2];
      res = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    }
    a.residual[(size_t)b * J + j] = res;
  }
  if (j < 3) a.global_trans_out[(size_t)b * 3 + j] = gt[j];
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_fit_pose(int32_t B, int32_t J, const float* joints, const int32_t* parents, const float* local_rot_in,
                   const float* global_trans_in, const float* targets, const float* weights, const uint8_t* locked,
                   int32_t iterations, int32_t cg_steps, float damping, float max_step, const float* extent, int32_t relative,
                   int32_t solve_translation, float* local_rot_out, float* global_trans_out, float* d_nodes, float* residual,
                   riggs_stream stream) {
  RIGGS_REQUIRE(B >= 1, "riggs_fit_pose: needs B >= 1");
  RIGGS_REQUIRE(J >= 1 && J <= MAX_J_WIDE, "riggs_fit_pose: num_joints must be in [1, 256]");
  RIGGS_REQUIRE(iterations >= 0 && cg_steps >= 1, "riggs_fit_pose: iterations >= 0 and cg_steps >= 1");
  RIGGS_REQUIRE((relative & ~3) == 0, "riggs_fit_pose: relative is a mask of bits 0 and 1");
  RIGGS_REQUIRE(damping > 0.f && max_step >= 0.f, "riggs_fit_pose: needs damping > 0 and max_step >= 0");  // (a NaN fails both)
  RIGGS_REQUIRE(joints && parents && local_rot_in && global_trans_in && targets && extent && local_rot_out && global_trans_out &&
                    d_nodes && residual, "riggs_fit_pose: NULL argument (extent is always needed: it scales the translation unknown)");
  FitArgs a;
  a.J = J; a.iterations = iterations; a.cg_steps = cg_steps; a.relative = relative; a.solve_translation = solve_translation != 0;
  a.damping = damping; a.max_step = max_step;
  a.joints = joints; a.parents = parents; a.local_rot_in = local_rot_in; a.global_trans_in = global_trans_in;
  a.targets = targets; a.weights = weights; a.locked = locked; a.extent = extent;
  a.local_rot_out = local_rot_out; a.global_trans_out = global_trans_out; a.d_nodes = d_nodes; a.residual = residual;
  if (J <= MAX_J) hipLaunchKernelGGL(fit_pose_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(fit_pose_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
