// Pose fitting to LINES (riggs_amd/pose_edit.py: fit_rays, fit_keypoints): a joint is held to up to RIGGS_RAYS_MAX lines in space
// (the ray through a camera centre and a 2-D keypoint, the editor's cursor) and / or to one point (a pin: fit.hip's target), and the
// rig's pose is turned so that the posed joints come to lie on them.  fit.hip's method: Levenberg-Marquardt with Buss & Kim's clamped
// step, the damped normal equations solved matrix-free by Jacobi-preconditioned conjugate gradients over the two tree sweeps.  The
// distance of a point to a line has the constant Jacobian I - d d^T with respect to the point, so fit.hip's scalar weight s_h^2
// becomes a symmetric 3 x 3 metric per joint that does not depend on the pose.  Restated from the published methods; the reference
// has nothing like it.  tests/rays_ref.py is the NumPy restatement this kernel is held to.
//
// Once per launch, thread h: a ray k is live iff w_hk > 0 and 0 < |d_hk| < inf (a NaN fails every comparison); d <- d / |d|; the
// pin is live iff wp_h > 0.  Nothing of a constraint that is not live is read beyond what decides that (the weight, then the
// direction).   N_h = wp_h I + sum_k w_hk (I - d_hk d_hk^T)  as 6 floats (xx yy zz xy xz yz), n_h = ((N_xx + N_yy) + N_zz) / 3.
// One iteration is fit.hip's (its header comment, steps 1-5) with
//   1  e_k = v - (d . v) d, v = o_k - posed_h (from the joint to the nearest point of the line); the pin: e = t - posed_h; each
//      shortened to max_step on its own;  f_h = sum_k w_hk e_k + wp_h e  (k ascending, the pin last);  b = J^T f
//   3  the moments S0, S1, S2 of n_h, n_h pc, n_h |pc|^2
//   4  down: u_h = (W_h x pc_h - C_h) + extent tau';  up: F, M over the subtrees of N_h u_h and pc_h x (N_h u_h)
// and the residual of a joint is the largest unclamped |e| over its live constraints (0 without any).
//
// ONE workgroup per problem, ALL iterations in one launch, thread j owns joint j, one wave64 up to 64 joints and 256 threads
// beyond: the frame of pose_solve.h and the barrier discipline of fit.hip, call for call.  The rays of a joint are used once per
// iteration (step 1), N_h in every CG step: N_h always lives in registers; the rays either live there as well (REGS: 7 floats a
// ray, every loop over them fully unrolled so that no array is indexed at run time) or are read again from global memory in every
// iteration (riggs_set_option("rays_reread", 1)): the same operations on the same values, the same bits.  No float atomics.
#include "pose_solve.h"

#include <cmath>

namespace riggs {

#define RAYS_CG_EPS 1e-10f  // (fit.hip's FIT_CG_EPS; tests/fit_ref.py: CG_EPS)

struct RaysArgs {
  SolveArgs s;
  int cg_steps, K;
  const float* origins; const float* directions; const float* ray_weights;
  const float* pins; const float* pin_weights;
};

template <bool WIDE>
struct RaysShared {  // (fit.hip's FitShared: one wave touches none of this)
  typename SolveChain<WIDE>::Shared fk;  // fk.A is the up-sweeps' row buffer
  float dn[WIDE ? MAX_J_WIDE : 1][8];    // the down-sweeps' row buffer
  float part[2][8];                      // a dot product's slot: the four waves' sums, then the root's four values
};

__device__ __forceinline__ float rays_dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void rays_cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// fit.hip's fit_dot: the workgroup's sum of `term`, the same bits in every thread; root[0..3] of thread 0 reaches every thread.
template <bool WIDE>
__device__ __forceinline__ float rays_dot(float term, float (&root)[4], RaysShared<WIDE>& ws, int& slot) {
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
    slot ^= 1;
    return sum;
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) root[e] = fk_lane_get(root[e], 0);
    return wave_sum_bcast(term);
  }
}

// Ray k of row (b, h): w = 0 where it is not live, else its weight, origin and unit direction.
__device__ __forceinline__ void ray_load(const RaysArgs& a, size_t row, int k, float& w, float (&o)[3], float (&d)[3]) {
  w = 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) { o[c] = 0.f; d[c] = 0.f; }
  const size_t i = row * a.K + k;
  const float wk = a.ray_weights[i];
  if (wk > 0.f) {  // (a NaN weight: off)
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = a.directions[i * 3 + c];
    const float len = sqrtf(rays_dot3(v, v));
    if (len > 0.f && len < INFINITY) {
      w = wk;
#pragma unroll
      for (int c = 0; c < 3; c++) { d[c] = v[c] / len; o[c] = a.origins[i * 3 + c]; }
    }
  }
}

// e: from `pos` to the nearest point of the line (o, unit d)
__device__ __forceinline__ void ray_error(const float (&o)[3], const float (&d)[3], const float (&pos)[3], float (&e)[3]) {
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; c++) v[c] = o[c] - pos[c];
  const float t = rays_dot3(d, v);
#pragma unroll
  for (int c = 0; c < 3; c++) e[c] = v[c] - t * d[c];
}

// f += w clamp(e, max_step); -> |e| before the clamp (clamped_step's arithmetic)
__device__ __forceinline__ float rays_force(float w, float (&e)[3], float max_step, float (&f)[3]) {
  const float len = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
  if (len > max_step) {
    const float k = max_step / len;
#pragma unroll
    for (int c = 0; c < 3; c++) e[c] = e[c] * k;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) f[c] = f[c] + w * e[c];
  return len;
}

template <bool WIDE, bool REGS>
__global__ __launch_bounds__(WIDE ? 256 : 64) void fit_rays_kernel(RaysArgs a) {
  constexpr int NJ = WIDE ? MAX_J_WIDE : MAX_J;
  constexpr int NR = REGS ? RIGGS_RAYS_MAX : 1;
  __shared__ float pos[NJ][3];  // posed joints of this iteration
  __shared__ RaysShared<WIDE> wsh;
  const int b = blockIdx.x, j = threadIdx.x;
  const int J = a.s.J, K = a.K;
  const bool on = j < J;
  const size_t row = (size_t)b * J + j;

  // ---- the problem's inputs (pose_solve.h), then the joint's constraints and their metric
  const float ext = a.s.extent[0];
  SolveIn pr;
  float gt[3];
  solve_load(a.s, b, j, ext, pr, gt);
  float wp = 0.f, tg[3] = {0.f, 0.f, 0.f};
  float rw[NR], ro[NR][3], rd[NR][3];
#pragma unroll
  for (int k = 0; k < NR; k++) {
    rw[k] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) { ro[k][c] = 0.f; rd[k][c] = 0.f; }
  }
  float N[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (on) {
    if (a.pins) {
      const float w = a.pin_weights[row];
      if (w > 0.f) {  // (a NaN weight: off)  a pin without weight is not read at all
        wp = w;
#pragma unroll
        for (int c = 0; c < 3; c++) tg[c] = a.pins[row * 3 + c];
      }
    }
    N[0] = wp; N[1] = wp; N[2] = wp;
#pragma unroll
    for (int k = 0; k < RIGGS_RAYS_MAX; k++) {
      if (k < K) {
        float w, o[3], d[3];
        ray_load(a, row, k, w, o, d);
        if (w > 0.f) {
          N[0] = N[0] + w * (1.f - d[0] * d[0]);
          N[1] = N[1] + w * (1.f - d[1] * d[1]);
          N[2] = N[2] + w * (1.f - d[2] * d[2]);
          N[3] = N[3] - w * (d[0] * d[1]);
          N[4] = N[4] - w * (d[0] * d[2]);
          N[5] = N[5] - w * (d[1] * d[2]);
        }
        if constexpr (REGS) {
          rw[k] = w;
#pragma unroll
          for (int c = 0; c < 3; c++) { ro[k][c] = o[c]; rd[k][c] = d[c]; }
        }
      }
    }
  }
  const float nh = ((N[0] + N[1]) + N[2]) / 3.f;
  const bool turn = on && !pr.locked;
  const float damping2 = pr.damping2;
  const bool trans = a.s.solve_translation != 0;
  int slot = 0;

  // ---- topology and the first sweep
  typedef SolveChain<WIDE> Chain;
  typename Chain::Fk f;
  Chain::forward(J, pr.in, f, wsh.fk);

  float worst = 0.f;  // the residual: of the last pass
  for (int it = 0;; it++) {
    if (it > 0) Chain::sweep(J, pr.in, f, wsh.fk);
    Chain::posed(f, wsh.fk, pr, gt, on, pos[j]);
    __syncthreads();
    const bool last = it >= a.s.iterations;

    // ---- 1: the clamped force of the joint's lines and pin (the last pass: their distances only)
    float fh0[3] = {0.f, 0.f, 0.f};
    worst = 0.f;
    if (on) {
      const float limit = last ? INFINITY : pr.max_step;
#pragma unroll
      for (int k = 0; k < RIGGS_RAYS_MAX; k++) {
        if (k < K) {
          float e[3];
          if constexpr (REGS) {
            if (rw[k] > 0.f) {
              ray_error(ro[k], rd[k], pos[j], e);
              worst = fmaxf(worst, rays_force(rw[k], e, limit, fh0));
            }
          } else {
            float w, o[3], d[3];
            ray_load(a, row, k, w, o, d);
            if (w > 0.f) {
              ray_error(o, d, pos[j], e);
              worst = fmaxf(worst, rays_force(w, e, limit, fh0));
            }
          }
        }
      }
      if (wp > 0.f) {
        float e[3];
#pragma unroll
        for (int c = 0; c < 3; c++) e[c] = tg[c] - pos[j][c];
        worst = fmaxf(worst, rays_force(wp, e, limit, fh0));
      }
    }
    if (last) break;

    float pc[3] = {0.f, 0.f, 0.f}, pv[3] = {0.f, 0.f, 0.f};
    if (on) {
#pragma unroll
      for (int c = 0; c < 3; c++) { pc[c] = pos[j][c] - pos[0][c]; pv[c] = pos[pr.in.par][c] - pos[0][c]; }
    }
    // ---- 3 (and b = J^T f): one up-sweep of F, M, S0, S1, S2
    float bq[3], minv;
    float root[4];
    {
      float v[11], mh[3];
      rays_cross3(pc, fh0, mh);
#pragma unroll
      for (int c = 0; c < 3; c++) { v[c] = fh0[c]; v[3 + c] = mh[c]; v[7 + c] = nh * pc[c]; }
      v[6] = nh;
      v[10] = nh * rays_dot3(pc, pc);
      if constexpr (WIDE) fk_block_subtree(J, f, wsh.fk, wsh.fk.A, v);
      else fk_wave_subtree(J, f, v);
      const float F[3] = {v[0], v[1], v[2]}, S1[3] = {v[7], v[8], v[9]};
      float pf[3];
      rays_cross3(pv, F, pf);
#pragma unroll
      for (int c = 0; c < 3; c++) bq[c] = turn ? v[3 + c] - pf[c] : 0.f;
      const float dd = fmaxf((v[10] - 2.f * rays_dot3(pv, S1)) + rays_dot3(pv, pv) * v[6], 0.f);
      minv = 1.f / ((2.f / 3.f) * dd + damping2);
      root[0] = v[0]; root[1] = v[1]; root[2] = v[2]; root[3] = v[6];
    }
    // ---- 4: PCG from x = 0
    float x[3] = {0.f, 0.f, 0.f}, r[3], z[3], p[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { r[c] = bq[c]; z[c] = minv * r[c]; p[c] = z[c]; }
    float rz = rays_dot(rays_dot3(r, z), root, wsh, slot);
    float xt[3] = {0.f, 0.f, 0.f}, rt[3] = {0.f, 0.f, 0.f}, zt[3] = {0.f, 0.f, 0.f}, pt[3] = {0.f, 0.f, 0.f}, minvt = 0.f;
    if (trans) {
      minvt = 1.f / ((ext * ext) * root[3] + damping2);
#pragma unroll
      for (int c = 0; c < 3; c++) { rt[c] = ext * root[c]; zt[c] = minvt * rt[c]; pt[c] = zt[c]; }
      rz = rz + rays_dot3(rt, zt);
    }
    const float rz0 = rz;
    for (int k = 0; k < a.cg_steps; k++) {
      if (!(rz > RAYS_CG_EPS * rz0)) break;  // (uniform: every thread holds the same rz)
      // down: W, C along the paths
      float u[3];
      {
        float v[6], c0[3];
        rays_cross3(p, pv, c0);
#pragma unroll
        for (int c = 0; c < 3; c++) { v[c] = p[c]; v[3 + c] = c0[c]; }
        if constexpr (WIDE) fk_block_prefix(J, f, wsh.dn, v);
        else fk_wave_prefix(f, v);
        const float W[3] = {v[0], v[1], v[2]};
        float wx[3];
        rays_cross3(W, pc, wx);
#pragma unroll
        for (int c = 0; c < 3; c++) u[c] = (wx[c] - v[3 + c]) + (trans ? ext * pt[c] : 0.f);
      }
      // up: F, M over the subtrees of N u
      float Ap[3], Apt[3] = {0.f, 0.f, 0.f};
      {
        float v[6], fh[3], mh[3];
        fh[0] = (N[0] * u[0] + N[3] * u[1]) + N[4] * u[2];
        fh[1] = (N[3] * u[0] + N[1] * u[1]) + N[5] * u[2];
        fh[2] = (N[4] * u[0] + N[5] * u[1]) + N[2] * u[2];
        rays_cross3(pc, fh, mh);
#pragma unroll
        for (int c = 0; c < 3; c++) { v[c] = fh[c]; v[3 + c] = mh[c]; }
        if constexpr (WIDE) fk_block_subtree(J, f, wsh.fk, wsh.fk.A, v);
        else fk_wave_subtree(J, f, v);
        const float F[3] = {v[0], v[1], v[2]};
        float pf[3];
        rays_cross3(pv, F, pf);
#pragma unroll
        for (int c = 0; c < 3; c++) Ap[c] = turn ? (v[3 + c] - pf[c]) + damping2 * p[c] : 0.f;
        root[0] = v[0]; root[1] = v[1]; root[2] = v[2]; root[3] = 0.f;
      }
      float pAp = rays_dot(rays_dot3(p, Ap), root, wsh, slot);
      if (trans) {
#pragma unroll
        for (int c = 0; c < 3; c++) Apt[c] = ext * root[c] + damping2 * pt[c];
        pAp = pAp + rays_dot3(pt, Apt);
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
      const float rzn = rays_dot(rays_dot3(r, z), root, wsh, slot) + rays_dot3(rt, zt);
      const float beta = rzn / rz;
#pragma unroll
      for (int c = 0; c < 3; c++) { p[c] = z[c] + beta * p[c]; pt[c] = zt[c] + beta * pt[c]; }
      rz = rzn;
    }
    // ---- 5: omega_a = x_a into the parent's frame, onto the quaternion
    const float dgt[3] = {ext * xt[0], ext * xt[1], ext * xt[2]};
    Chain::turn(f, wsh.fk, x, turn, trans, dgt, pr, gt);
  }

  // ---- the result (pos is the posed skeleton of the final quaternions, behind a barrier)
  solve_write(a.s, b, j, pr, gt, pos);
  if (on) a.s.residual[row] = worst;
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_fit_rays(int32_t B, int32_t J, int32_t K, const float* joints, const int32_t* parents, const float* local_rot_in,
                   const float* global_trans_in, const float* origins, const float* directions, const float* ray_weights,
                   const float* pins, const float* pin_weights, const uint8_t* locked, int32_t iterations, int32_t cg_steps,
                   float damping, float max_step, const float* extent, int32_t relative, int32_t solve_translation,
                   float* local_rot_out, float* global_trans_out, float* d_nodes, float* residual, riggs_stream stream) {
  RaysArgs a;
  if (int rc = solve_args("riggs_fit_rays", B, J, joints, parents, local_rot_in, global_trans_in, locked, iterations, damping, max_step,
                          extent, relative, solve_translation, local_rot_out, global_trans_out, d_nodes, residual, a.s)) return rc;
  RIGGS_REQUIRE(K >= 0 && K <= RIGGS_RAYS_MAX, "riggs_fit_rays: K must be in [0, RIGGS_RAYS_MAX]");
  RIGGS_REQUIRE(cg_steps >= 1, "riggs_fit_rays: cg_steps >= 1");
  RIGGS_REQUIRE(extent, "riggs_fit_rays: NULL argument (extent is always needed: it scales the translation unknown)");
  RIGGS_REQUIRE(K == 0 || (origins && directions && ray_weights), "riggs_fit_rays: K > 0 needs origins, directions and ray_weights");
  RIGGS_REQUIRE((pins != nullptr) == (pin_weights != nullptr), "riggs_fit_rays: pins and pin_weights come together");
  RIGGS_REQUIRE(K > 0 || pins, "riggs_fit_rays: K == 0 needs pins");
  a.cg_steps = cg_steps; a.K = K;
  a.origins = origins; a.directions = directions; a.ray_weights = ray_weights; a.pins = pins; a.pin_weights = pin_weights;
  const bool reread = option(OPT_RAYS_REREAD) != 0;
  const dim3 grid(B);
  hipStream_t s = (hipStream_t)stream;
  if (J <= MAX_J) {
    if (reread) hipLaunchKernelGGL((fit_rays_kernel<false, false>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((fit_rays_kernel<false, true>), grid, dim3(64), 0, s, a);
  } else {
    if (reread) hipLaunchKernelGGL((fit_rays_kernel<true, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((fit_rays_kernel<true, true>), grid, dim3(256), 0, s, a);
  }
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
