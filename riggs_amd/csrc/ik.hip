// Inverse kinematics on the rig's own chain (riggs_amd/pose_edit.py: solve_ik): drag up to 8 handle joints towards targets and
// let the chain follow.  Damped least squares (Wampler 1986) with the clamped target step of Buss & Kim (Selectively damped
// least squares for inverse kinematics, 2005, section 3), restated from the published method; the reference has no IK.
// tests/ik_ref.py is the NumPy restatement this kernel is held to.
//
// Kinematics (fk_device.h; skeleton_utils/skeleton_warp.py:242-273): joint j's quaternion turns joint j about its PARENT's rest
// position, the root about itself; vp(j) = parents[j], vp(0) = 0.  One iteration:
//   1  FK: G_j, posed_j = G_j [x_j; 1] + gt; joint a's pivot in the world is piv_a = posed_vp(a)
//   2  per live handle e on joint h: d = target_e - posed_h, shortened to max_step; s = sqrt(w_e), r_e = s d
//   3  J_{e,a} = -s [posed_h - piv_a]x for the unlocked joints a on the path root .. h (h included), else 0; with
//      solve_translation a further block s I
//   4  A = J J^T + damping^2 I (3E x 3E), A y = r by Cholesky; omega_a = J_{.,a}^T y, dgt = sum_e s y_e
//   5  delta_a = R(G_vp(a))^T omega_a (the root: omega_0), theta = |delta_a|; theta > 0: q_a <- (cos theta/2, sin(theta/2) delta_a / theta) (x) q_a
// and one more FK behind the last iteration for d_nodes and the residual.  The inputs, 1, the clamped step of 2, 5 and the result
// are the frame this solver shares with fit.hip: pose_solve.h has them, here are 3 and 4.
//
// ONE workgroup per problem, ALL iterations in one launch: thread j owns joint j and keeps its quaternion in registers.
// J <= 64: one wave64 on fk_wave_*; 65 .. 256: 256 threads on fk_block_*.  The topology (levels, children; each handle's ancestor
// set as a 256-bit mask in LDS, folded into 8 bits per thread: "my joint turns handle e") is computed once, only the level sweep
// repeats.  With p_e = posed_h - piv_a the blocks of J J^T are  s_e s_f sum_a ((p_e . p_f) I - p_f p_e^T)  over the joints both
// paths share: every thread forms its term, a wave adds its 64 with DPP row operations (common.h: wave_sum, a fixed tree), lane
// 63 leaves the sum in LDS and the (up to four) waves' sums are added in wave order.  No float atomics: the same inputs give the
// same bits on every run, and a problem never reads its neighbours in the batch.  The 3E x 3E Cholesky (left-looking, row i on
// lane i of wave 0, the factor in LDS) and the two triangular solves (the right-hand side in registers, the pivot row by lane
// shuffle) follow; their barriers are passed by every thread of the workgroup.
// What bounds it is the chain of dependent steps (depth levels per sweep, 3E steps per factorisation and per solve, times the
// iterations), not bytes: a problem reads and writes a few KiB once.
#include "pose_solve.h"

namespace riggs {

#define IK_MAX_E RIGGS_IK_MAX_HANDLES
#define IK_MAX_N (3 * IK_MAX_E)

struct IkArgs {
  SolveArgs s;
  int E;
  const int32_t* handles; const float* targets; const float* weights;
};

struct IkShared {
  float pos[MAX_J_WIDE][3];                      // posed joints of this iteration
  float part[4][IK_MAX_E * IK_MAX_E][9];         // per wave: the 3 x 3 sums of the handle pairs e <= f (at e * IK_MAX_E + f)
  float A[IK_MAX_N][IK_MAX_N + 1];               // J J^T + damping^2 I, then its Cholesky factor in the lower triangle
  float rhs[IK_MAX_N], y[IK_MAX_N];
  uint32_t path[IK_MAX_E][FK_WIDE_WORDS];        // the joints root .. handle
  int par[MAX_J_WIDE];
  int handle[IK_MAX_E], live[IK_MAX_E];          // the handle's joint (-1: an index outside [0, J)); weight > 0 and a valid index
  float s[IK_MAX_E], target[IK_MAX_E][3];
};

template <bool WIDE>
__global__ __launch_bounds__(WIDE ? 256 : 64) void ik_solve_kernel(IkArgs a) {
  constexpr int NT = WIDE ? 256 : 64, NW = NT / RIGGS_WAVE;
  __shared__ IkShared sh;
  __shared__ typename SolveChain<WIDE>::Shared wsh;
  const int b = blockIdx.x, j = threadIdx.x, lane = j & (RIGGS_WAVE - 1), wave = j / RIGGS_WAVE;
  const int J = a.s.J, E = a.E, n = 3 * E;
  const bool on = j < J;

  // ---- the problem's inputs (the parents clamped: the walks below end); extent == NULL: 1
  SolveIn pr;
  float gt[3];
  solve_load(a.s, b, j, a.s.extent ? a.s.extent[0] : 1.f, pr, gt);
  for (int i = j; i < MAX_J_WIDE; i += NT) sh.par[i] = 0;
  __syncthreads();
  if (on) sh.par[j] = pr.in.par;
  if (j < IK_MAX_E) {
    int h = -1, live = 0;
    float s = 0.f;
    if (j < E) {
      h = a.handles[(size_t)b * E + j];
      if (h < 0 || h >= J) h = -1;
      const float w = a.weights ? a.weights[(size_t)b * E + j] : 1.f;
      live = (h >= 0 && w > 0.f) ? 1 : 0;
      s = live ? sqrtf(w) : 0.f;
    }
    sh.handle[j] = h; sh.live[j] = live; sh.s[j] = s;
#pragma unroll
    for (int c = 0; c < 3; c++) sh.target[j][c] = (j < E) ? a.targets[((size_t)b * E + j) * 3 + c] : 0.f;
#pragma unroll
    for (int w = 0; w < FK_WIDE_WORDS; w++) sh.path[j][w] = 0u;
  }
  __syncthreads();
  if (j < E && sh.live[j]) {  // thread e walks handle e's ancestors: par[i] < i, so at most J - 1 steps
    int i = sh.handle[j];
    for (int step = 0; step < MAX_J_WIDE; step++) {
      sh.path[j][i >> 5] |= 1u << (i & 31);
      if (i == 0) break;
      i = sh.par[i];
    }
  }
  __syncthreads();
  uint32_t mine = 0u;  // bit e: this thread's joint turns handle e
#pragma unroll
  for (int e = 0; e < IK_MAX_E; e++)
    if (e < E && on && !pr.locked && (sh.path[e][j >> 5] >> (j & 31) & 1u)) mine |= 1u << e;

  // ---- topology and the first sweep
  typedef SolveChain<WIDE> Chain;
  typename Chain::Fk f;
  Chain::forward(J, pr.in, f, wsh);

  for (int it = 0;; it++) {
    if (it > 0) Chain::sweep(J, pr.in, f, wsh);
    Chain::posed(f, wsh, pr, gt, on, sh.pos[j]);
    __syncthreads();
    if (it >= a.s.iterations) break;

    // ---- 2: the right-hand side, one thread per handle
    if (j < IK_MAX_E) {
      float r[3] = {0.f, 0.f, 0.f};
      if (j < E && sh.live[j]) clamped_step(sh.target[j], sh.pos[sh.handle[j]], pr.max_step, sh.s[j], r);
#pragma unroll
      for (int c = 0; c < 3; c++) sh.rhs[3 * j + c] = r[c];
    }
    // ---- 3: p_e = posed_h - piv_a for the handles this joint turns, and the sums of J J^T over the joints
    float p[IK_MAX_E][3];
    {
      float piv[3];
#pragma unroll
      for (int c = 0; c < 3; c++) piv[c] = sh.pos[pr.in.par][c];
#pragma unroll
      for (int e = 0; e < IK_MAX_E; e++) {
        const int h = (mine >> e & 1u) ? sh.handle[e] : 0;
#pragma unroll
        for (int c = 0; c < 3; c++) p[e][c] = (mine >> e & 1u) ? sh.pos[h][c] - piv[c] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < IK_MAX_E; e++)
#pragma unroll
      for (int g = e; g < IK_MAX_E; g++) {
        if (g < E) {  // (uniform: every lane of the wave adds)
          const bool both = (mine >> e & 1u) && (mine >> g & 1u);
          const float dot = p[e][0] * p[g][0] + p[e][1] * p[g][1] + p[e][2] * p[g][2];
#pragma unroll
          for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
              float v = both ? ((r == c ? dot : 0.f) - p[g][r] * p[e][c]) : 0.f;
              v = wave_sum(v);
              if (lane == RIGGS_WAVE - 1) sh.part[wave][e * IK_MAX_E + g][3 * r + c] = v;
            }
        }
      }
    __syncthreads();
    // ---- 4: A (block (f, e) below the diagonal is block (e, f) transposed), its factor, the two solves
    for (int t = j; t < n * n; t += NT) {
      const int row = t / n, col = t - row * n;
      const int e = row / 3, r = row - 3 * e, g = col / 3, c = col - 3 * g;
      float v = 0.f;
      for (int w = 0; w < NW; w++) v += (e <= g) ? sh.part[w][e * IK_MAX_E + g][3 * r + c] : sh.part[w][g * IK_MAX_E + e][3 * c + r];
      const float ss = sh.s[e] * sh.s[g];
      v = ss * v;
      if (a.s.solve_translation && r == c) v += ss;
      if (row == col) v += pr.damping2;
      sh.A[row][col] = v;
    }
    __syncthreads();
    const bool rowon = j < n;  // (wave 0: n <= 24)
    for (int k = 0; k < n; k++) {
      float v = 0.f;
      if (rowon && j >= k) {
        v = sh.A[j][k];
        for (int m = 0; m < k; m++) v -= sh.A[j][m] * sh.A[k][m];
      }
      const float lkk = sqrtf(__shfl(v, k));
      if (rowon && j >= k) sh.A[j][k] = (j == k) ? lkk : v / lkk;
      __syncthreads();
    }
    float bb = rowon ? sh.rhs[j] : 0.f;
    for (int k = 0; k < n; k++) {  // L z = r
      const float zk = __shfl(bb, k) / sh.A[k][k];
      if (rowon && j > k) bb -= sh.A[j][k] * zk;
      else if (j == k) bb = zk;
    }
    for (int k = n - 1; k >= 0; k--) {  // L^T y = z
      const float yk = __shfl(bb, k) / sh.A[k][k];
      if (rowon && j < k) bb -= sh.A[k][j] * yk;
      else if (j == k) bb = yk;
    }
    if (rowon) sh.y[j] = bb;
    __syncthreads();
    // ---- 5: omega_a = sum_e s_e p_e x y_e, into the parent's frame, onto the quaternion
    float om[3] = {0.f, 0.f, 0.f}, dgt[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < IK_MAX_E; e++) {
      if (e < E) {
        const float s = sh.s[e], y0 = sh.y[3 * e], y1 = sh.y[3 * e + 1], y2 = sh.y[3 * e + 2];
        if (mine >> e & 1u) {
          om[0] = om[0] + s * (p[e][1] * y2 - p[e][2] * y1);
          om[1] = om[1] + s * (p[e][2] * y0 - p[e][0] * y2);
          om[2] = om[2] + s * (p[e][0] * y1 - p[e][1] * y0);
        }
        if (sh.live[e]) { dgt[0] = dgt[0] + s * y0; dgt[1] = dgt[1] + s * y1; dgt[2] = dgt[2] + s * y2; }
      }
    }
    Chain::turn(f, wsh, om, on && mine != 0u, a.s.solve_translation != 0, dgt, pr, gt);
  }

  // ---- the result (sh.pos is the posed skeleton of the final quaternions, behind a barrier)
  solve_write(a.s, b, j, pr, gt, sh.pos);
  if (j < E) {
    const int h = sh.handle[j];  // (a handle index outside [0, J): there is no position to measure)
    a.s.residual[(size_t)b * E + j] = h >= 0 ? solve_distance(sh.target[j], sh.pos[h]) : __builtin_nanf("");
  }
}

}  // namespace riggs

using namespace riggs;

extern "C" {

int riggs_ik_solve(int32_t B, int32_t J, int32_t E, const float* joints, const int32_t* parents, const float* local_rot_in,
                   const float* global_trans_in, const int32_t* handles, const float* targets, const float* weights,
                   const uint8_t* locked, int32_t iterations, float damping, float max_step, const float* extent, int32_t relative,
                   int32_t solve_translation, float* local_rot_out, float* global_trans_out, float* d_nodes, float* residual,
                   riggs_stream stream) {
  IkArgs a;
  if (int rc = solve_args("riggs_ik_solve", B, J, joints, parents, local_rot_in, global_trans_in, locked, iterations, damping, max_step,
                          extent, relative, solve_translation, local_rot_out, global_trans_out, d_nodes, residual, a.s)) return rc;
  RIGGS_REQUIRE(E >= 1 && E <= IK_MAX_E, "riggs_ik_solve: 1 to RIGGS_IK_MAX_HANDLES handles");
  RIGGS_REQUIRE(relative == 0 || extent, "riggs_ik_solve: a relative damping or max_step needs extent");
  RIGGS_REQUIRE(handles && targets, "riggs_ik_solve: NULL argument");
  a.E = E; a.handles = handles; a.targets = targets; a.weights = weights;
  if (J <= MAX_J) hipLaunchKernelGGL(ik_solve_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(ik_solve_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
