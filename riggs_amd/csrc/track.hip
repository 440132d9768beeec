// Filters along the time axis of a pose track (riggs_amd/track.py; include/riggs_hip.h has the method, step by step).
//   riggs_track_smooth    confidence-weighted Gaussian window on SO(3): the chordal L2 mean of the window's rotations (Markley,
//                         Cheng, Crassidis & Oshman 2007: the dominant eigenvector of sum w q q^T), cyclic Jacobi in registers
//   riggs_track_one_euro  the one-euro filter (Casiez, Roussel & Vogel 2012) on unit quaternions and on the root translation
// Inference only.  No float atomics, no synchronisation, no allocation: both are legal inside a stream capture, the same inputs give
// the same bits, and a track's result does not depend on the rest of the batch.
// Built with FP contraction off: tests/track_ref.py rounds every operation, its float32 form is the yardstick for the rounding here.
#include "common.h"

namespace riggs {

#define TRACK_SWEEPS 4  // cyclic Jacobi sweeps over the six pairs of the 4 x 4 matrix: fixed, no data-dependent exit

struct Quat {
  float e[4];
};

__device__ __forceinline__ Quat load_quat(const float* p) {
  const float4 v = *reinterpret_cast<const float4*>(p);  // (16-byte aligned: the entry checks the base, a row is 4 floats)
  Quat q;
  q.e[0] = v.x; q.e[1] = v.y; q.e[2] = v.z; q.e[3] = v.w;
  return q;
}
__device__ __forceinline__ void store_quat(float* p, const Quat& q) {
  *reinterpret_cast<float4*>(p) = make_float4(q.e[0], q.e[1], q.e[2], q.e[3]);
}
__device__ __forceinline__ float dot4(const Quat& a, const Quat& b) {
  return ((a.e[0] * b.e[0] + a.e[1] * b.e[1]) + a.e[2] * b.e[2]) + a.e[3] * b.e[3];
}
// q / |q| where 0 < |q|^2 < inf in float32; false (and q untouched) otherwise: a zero, NaN, infinite or overflowing sample
__device__ __forceinline__ bool normalise(Quat& q) {
  const float n2 = dot4(q, q);
  if (!(n2 > 0.0f && n2 < INFINITY)) return false;
  const float n = sqrtf(n2);
#pragma unroll
  for (int e = 0; e < 4; e++) q.e[e] = q.e[e] / n;
  return true;
}
__device__ __forceinline__ bool finite3(const float* p) { return fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY; }

// ------------------------------------------------------------------------------------------------ the Gaussian window
struct SmoothArgs {
  int B, T, J, R, wrap;
  const float *rot, *trans, *w, *tw, *taps;  // (B,T,J,4), (B,T,3) or NULL, (B,T,J) or NULL, (B,T) or NULL, (R + 1)
  float *rot_out, *trans_out, *support;      // (B,T,J,4), (B,T,3) or NULL, (B,T,J)
};

// The unit eigenvector of the largest eigenvalue of the symmetric a (both halves given); on equal eigenvalues the first column.
__device__ __forceinline__ Quat dominant_eigenvector(float (&a)[4][4]) {
  float v[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) v[r][c] = r == c ? 1.0f : 0.0f;
#pragma unroll
  for (int sweep = 0; sweep < TRACK_SWEEPS; sweep++) {
#pragma unroll
    for (int p = 0; p < 3; p++) {
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        // the rotation that zeroes a[p][q] (Jacobi 1846; the smaller root of t^2 + 2 t theta - 1 = 0); t = 0 where it is zero already
        const float apq = a[p][q];
        const float theta = (a[q][q] - a[p][p]) / (2.0f * apq);
        const float tt = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
        const float t = apq != 0.0f ? (theta < 0.0f ? -tt : tt) : 0.0f;
        const float c = 1.0f / sqrtf(t * t + 1.0f);
        const float s = t * c;
        a[p][p] = a[p][p] - t * apq;
        a[q][q] = a[q][q] + t * apq;
        a[p][q] = a[q][p] = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          if (r != p && r != q) {
            const float arp = a[r][p], arq = a[r][q];
            a[r][p] = a[p][r] = c * arp - s * arq;
            a[r][q] = a[q][r] = s * arp + c * arq;
          }
          const float vrp = v[r][p], vrq = v[r][q];
          v[r][p] = c * vrp - s * vrq;
          v[r][q] = s * vrp + c * vrq;
        }
      }
    }
  }
  float best = a[0][0];
  Quat out;
#pragma unroll
  for (int e = 0; e < 4; e++) out.e[e] = v[e][0];
#pragma unroll
  for (int k = 1; k < 4; k++) {
    const bool take = a[k][k] > best;
    best = take ? a[k][k] : best;
#pragma unroll
    for (int e = 0; e < 4; e++) out.e[e] = take ? v[e][k] : out.e[e];
  }
  const float n = sqrtf(dot4(out, out));  // (orthonormal up to the sweeps' rounding: n is 1 within a few ulp)
#pragma unroll
  for (int e = 0; e < 4; e++) out.e[e] = out.e[e] / n;
  return out;
}

// One thread per (b, t, j), adjacent threads on adjacent joints: a window step is one coalesced 16-byte load per lane.  The threads
// of joint 0 also filter the frame's translation.  The taps sit in LDS.
__global__ __launch_bounds__(256) void track_smooth_kernel(SmoothArgs a) {
  __shared__ float g[RIGGS_TRACK_MAX_RADIUS + 1];
  for (int d = threadIdx.x; d <= a.R; d += 256) g[d] = a.taps[d];
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.B * a.T * a.J) return;
  const int j = (int)(i % a.J);
  const int t = (int)((i / a.J) % a.T);
  const long long b = i / ((long long)a.J * a.T);
  const long long frame0 = b * a.T;  // the track's first frame among all frames
  const int lo = a.wrap ? -a.R : max(-a.R, -t), hi = a.wrap ? a.R : min(a.R, a.T - 1 - t);

  float m[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) m[r][c] = 0.0f;
  float sup = 0.0f;
  bool centre = false;
  Quat qc = {{1.0f, 0.0f, 0.0f, 0.0f}};
  for (int d = lo; d <= hi; d++) {
    int s = t + d;
    if (s < 0) s += a.T;  // (wrap only: 2 R + 1 <= T, so one step brings it back)
    if (s >= a.T) s -= a.T;
    const long long at = (frame0 + s) * a.J + j;
    const float c = a.w ? a.w[at] : 1.0f;
    if (!(c > 0.0f)) continue;  // a gap by its confidence (NaN fails the comparison): its quaternion is not read
    Quat q = load_quat(a.rot + 4 * at);
    if (!normalise(q)) continue;  // a gap by its quaternion
    const float wgt = g[d < 0 ? -d : d] * c;
    sup = sup + wgt;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float wq = wgt * q.e[r];
#pragma unroll
      for (int cc = r; cc < 4; cc++) m[r][cc] = m[r][cc] + wq * q.e[cc];
    }
    if (d == 0) { centre = true; qc = q; }
  }
  Quat out;
  if (sup > 0.0f) {
#pragma unroll
    for (int r = 1; r < 4; r++)
#pragma unroll
      for (int c = 0; c < r; c++) m[r][c] = m[c][r];
    out = dominant_eigenvector(m);
    bool flip;
    if (centre) {
      flip = dot4(out, qc) < 0.0f;
    } else {  // the first non-zero component positive
      const float lead = out.e[0] != 0.0f ? out.e[0] : out.e[1] != 0.0f ? out.e[1] : out.e[2] != 0.0f ? out.e[2] : out.e[3];
      flip = lead < 0.0f;
    }
    if (flip) {
#pragma unroll
      for (int e = 0; e < 4; e++) out.e[e] = -out.e[e];
    }
  } else {  // no support: the input sample normalised, or the identity
    sup = 0.0f;
    out = load_quat(a.rot + 4 * ((frame0 + t) * a.J + j));
    if (!normalise(out)) { out.e[0] = 1.0f; out.e[1] = out.e[2] = out.e[3] = 0.0f; }
  }
  store_quat(a.rot_out + 4 * i, out);
  a.support[i] = sup;

  if (j == 0 && a.trans) {
    float acc[3] = {0.0f, 0.0f, 0.0f}, ts = 0.0f;
    for (int d = lo; d <= hi; d++) {
      int s = t + d;
      if (s < 0) s += a.T;
      if (s >= a.T) s -= a.T;
      const float c = a.tw ? a.tw[frame0 + s] : 1.0f;
      if (!(c > 0.0f)) continue;
      const float* p = a.trans + 3 * (frame0 + s);
      if (!finite3(p)) continue;
      const float wgt = g[d < 0 ? -d : d] * c;
      ts = ts + wgt;
#pragma unroll
      for (int e = 0; e < 3; e++) acc[e] = acc[e] + wgt * p[e];
    }
    const float* p = a.trans + 3 * (frame0 + t);
    float* o = a.trans_out + 3 * (frame0 + t);
#pragma unroll
    for (int e = 0; e < 3; e++) o[e] = ts > 0.0f ? acc[e] / ts : p[e];
  }
}

// ------------------------------------------------------------------------------------------------ the one-euro filter
struct EuroArgs {
  int B, T, J;
  const float *rot, *trans, *w, *tw;  // (B,T,J,4), (B,T,3) or NULL, (B,T,J) or NULL, (B,T) or NULL
  float rate, min_cutoff, beta, d_cutoff, t_min_cutoff, t_beta;
  float *s_rot, *s_omega, *s_trans, *s_vel;  // state, read and written: (B,J,4), (B,J), (B,3), (B,3)
  int32_t *s_gap, *s_tgap;                   // (B,J), (B)
  float *rot_out, *trans_out;                // (B,T,J,4), (B,T,3) or NULL
};

// alpha(f, dt) = 1 / (1 + 1 / (2 pi f dt)); f = 0 gives 0
__device__ __forceinline__ float euro_alpha(float f, float dt) {
  const float r = (6.2831855f * f) * dt;
  return 1.0f / (1.0f + 1.0f / r);
}

// One lane per (b, j) walks the T frames, adjacent lanes on adjacent joints; the next frame's sample is in flight while this one is
// filtered (its address does not depend on the state).  The translations walk in blocks of their own behind the rotations' blocks,
// one lane per track: in a wave of joints the two walks would run one after the other.
__global__ __launch_bounds__(256) void track_one_euro_kernel(EuroArgs a) {
  const long long rot_lanes = (long long)a.B * a.J, rot_blocks = (rot_lanes + 255) / 256;
  if (blockIdx.x < rot_blocks) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rot_lanes) return;
    const int j = (int)(i % a.J);
    const long long b = i / a.J;
    const long long frame0 = b * a.T;
    const long long sj = b * a.J + j;
    Quat f = load_quat(a.s_rot + 4 * sj);
    float om = a.s_omega[sj];
    int gap = a.s_gap[sj];
    long long at = frame0 * a.J + j;
    float c = a.w ? a.w[at] : 1.0f;
    Quat x = load_quat(a.rot + 4 * at);
    for (int t = 0; t < a.T; t++) {
      const float c_now = c;
      Quat q = x;
      const long long here = at;
      if (t + 1 < a.T) {
        at += a.J;
        c = a.w ? a.w[at] : 1.0f;
        x = load_quat(a.rot + 4 * at);
      }
      if (c_now > 0.0f && normalise(q)) {
        if (gap < 0) {  // the first sample
          f = q;
          om = 0.0f;
        } else {
          const float dt = (float)(gap + 1) / a.rate;
          float dot = dot4(q, f);
          if (dot < 0.0f) {
#pragma unroll
            for (int e = 0; e < 4; e++) q.e[e] = -q.e[e];
          }
          dot = fminf(fabsf(dot), 1.0f);
          const float th = acosf(dot), sn = sinf(th);
          const float speed = (2.0f * th) / dt;
          const float ad = euro_alpha(a.d_cutoff, dt);
          om = ad * speed + (1.0f - ad) * om;
          const float al = euro_alpha(a.min_cutoff + a.beta * om, dt);
          // slerp_batch's steps from its dot product on (csrc/playback.hip): the linear weights where sin(theta) <= 1e-6
          float w0 = 1.0f - al, w1 = al;
          if (sn > 1e-6f) {
            w0 = sinf((1.0f - al) * th) / sn;
            w1 = sinf(al * th) / sn;
          }
          Quat r;
#pragma unroll
          for (int e = 0; e < 4; e++) r.e[e] = w0 * f.e[e] + w1 * q.e[e];
          const float nr = sqrtf(dot4(r, r));
#pragma unroll
          for (int e = 0; e < 4; e++) f.e[e] = r.e[e] / nr;
        }
        gap = 0;
      } else if (gap >= 0 && gap < 0x7fffffff - 1) {
        gap++;
      }
      Quat o = f;
      if (gap < 0) { o.e[0] = 1.0f; o.e[1] = o.e[2] = o.e[3] = 0.0f; }
      store_quat(a.rot_out + 4 * here, o);
    }
    store_quat(a.s_rot + 4 * sj, f);
    a.s_omega[sj] = om;
    a.s_gap[sj] = gap;
  } else {
    const long long b = ((long long)blockIdx.x - rot_blocks) * 256 + threadIdx.x;
    if (b >= a.B) return;
    const long long frame0 = b * a.T;
    float f[3], v[3];
#pragma unroll
    for (int e = 0; e < 3; e++) { f[e] = a.s_trans[3 * b + e]; v[e] = a.s_vel[3 * b + e]; }
    int gap = a.s_tgap[b];
    for (int t = 0; t < a.T; t++) {
      const float c = a.tw ? a.tw[frame0 + t] : 1.0f;
      const float* p = a.trans + 3 * (frame0 + t);
      float* o = a.trans_out + 3 * (frame0 + t);
      if (c > 0.0f && finite3(p)) {
        if (gap < 0) {
#pragma unroll
          for (int e = 0; e < 3; e++) { f[e] = p[e]; v[e] = 0.0f; }
        } else {
          const float dt = (float)(gap + 1) / a.rate;
          const float ad = euro_alpha(a.d_cutoff, dt);
#pragma unroll
          for (int e = 0; e < 3; e++) v[e] = ad * ((p[e] - f[e]) / dt) + (1.0f - ad) * v[e];
          const float speed = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
          const float al = euro_alpha(a.t_min_cutoff + a.t_beta * speed, dt);
#pragma unroll
          for (int e = 0; e < 3; e++) f[e] = al * p[e] + (1.0f - al) * f[e];
        }
        gap = 0;
      } else if (gap >= 0 && gap < 0x7fffffff - 1) {
        gap++;
      }
#pragma unroll
      for (int e = 0; e < 3; e++) o[e] = gap < 0 ? 0.0f : f[e];  // before any sample: the origin
    }
#pragma unroll
    for (int e = 0; e < 3; e++) { a.s_trans[3 * b + e] = f[e]; a.s_vel[3 * b + e] = v[e]; }
    a.s_tgap[b] = gap;
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace riggs

using namespace riggs;

extern "C" int riggs_track_smooth(int32_t B, int32_t T, int32_t J, int32_t radius, int32_t wrap, const float* rot_in,
                                  const float* trans_in, const float* weights, const float* trans_weights, const float* taps,
                                  float* rot_out, float* trans_out, float* support, riggs_stream stream) {
  RIGGS_REQUIRE(B >= 0 && T >= 0, "riggs_track_smooth: negative count");
  RIGGS_REQUIRE(J >= 1 && J <= RIGGS_TRACK_MAX_JOINTS, "riggs_track_smooth: 1 to RIGGS_TRACK_MAX_JOINTS joints");
  RIGGS_REQUIRE(radius >= 0 && radius <= RIGGS_TRACK_MAX_RADIUS, "riggs_track_smooth: radius must be in [0, RIGGS_TRACK_MAX_RADIUS]");
  RIGGS_REQUIRE(!wrap || T == 0 || 2 * radius + 1 <= T, "riggs_track_smooth: wrap needs 2 radius + 1 <= T");
  RIGGS_REQUIRE((trans_in == nullptr) == (trans_out == nullptr), "riggs_track_smooth: trans_in and trans_out come together");
  RIGGS_REQUIRE(trans_in || !trans_weights, "riggs_track_smooth: trans_weights without a translation");
  const long long total = (long long)B * T * J;
  if (total == 0) return 0;
  RIGGS_REQUIRE(rot_in && taps && rot_out && support, "riggs_track_smooth: NULL argument");
  RIGGS_REQUIRE(aligned16(rot_in) && aligned16(rot_out), "riggs_track_smooth: the quaternions must be 16-byte aligned");
  RIGGS_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "riggs_track_smooth: too many samples");
  SmoothArgs a;
  a.B = B; a.T = T; a.J = J; a.R = radius; a.wrap = wrap ? 1 : 0;
  a.rot = rot_in; a.trans = trans_in; a.w = weights; a.tw = trans_weights; a.taps = taps;
  a.rot_out = rot_out; a.trans_out = trans_out; a.support = support;
  hipLaunchKernelGGL(track_smooth_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int riggs_track_one_euro(int32_t B, int32_t T, int32_t J, const float* rot_in, const float* trans_in, const float* weights,
                                    const float* trans_weights, float rate, float min_cutoff, float beta, float d_cutoff,
                                    float trans_min_cutoff, float trans_beta, float* state_rot, float* state_omega,
                                    int32_t* state_gap, float* state_trans, float* state_velocity, int32_t* state_trans_gap,
                                    float* rot_out, float* trans_out, riggs_stream stream) {
  RIGGS_REQUIRE(B >= 0 && T >= 0, "riggs_track_one_euro: negative count");
  RIGGS_REQUIRE(J >= 1 && J <= RIGGS_TRACK_MAX_JOINTS, "riggs_track_one_euro: 1 to RIGGS_TRACK_MAX_JOINTS joints");
  RIGGS_REQUIRE(rate > 0.0f && rate < INFINITY, "riggs_track_one_euro: rate must be positive and finite");
  RIGGS_REQUIRE(min_cutoff > 0.0f && min_cutoff < INFINITY && d_cutoff > 0.0f && d_cutoff < INFINITY && beta >= 0.0f && beta < INFINITY,
                "riggs_track_one_euro: min_cutoff > 0, d_cutoff > 0, beta >= 0, all finite");
  RIGGS_REQUIRE(trans_min_cutoff > 0.0f && trans_min_cutoff < INFINITY && trans_beta >= 0.0f && trans_beta < INFINITY,
                "riggs_track_one_euro: trans_min_cutoff > 0, trans_beta >= 0, both finite");
  RIGGS_REQUIRE((trans_in == nullptr) == (trans_out == nullptr), "riggs_track_one_euro: trans_in and trans_out come together");
  RIGGS_REQUIRE(trans_in || !trans_weights, "riggs_track_one_euro: trans_weights without a translation");
  if (B == 0 || T == 0) return 0;
  RIGGS_REQUIRE(rot_in && rot_out && state_rot && state_omega && state_gap, "riggs_track_one_euro: NULL argument");
  RIGGS_REQUIRE(!trans_in || (state_trans && state_velocity && state_trans_gap), "riggs_track_one_euro: a translation needs its state");
  RIGGS_REQUIRE(aligned16(rot_in) && aligned16(rot_out) && aligned16(state_rot), "riggs_track_one_euro: the quaternions must be 16-byte aligned");
  const long long blocks = ((long long)B * J + 255) / 256 + (trans_in ? ((long long)B + 255) / 256 : 0);  // rotations, then translations
  RIGGS_REQUIRE(blocks <= 0x7fffffffLL, "riggs_track_one_euro: too many tracks");
  EuroArgs a;
  a.B = B; a.T = T; a.J = J; a.rot = rot_in; a.trans = trans_in; a.w = weights; a.tw = trans_weights;
  a.rate = rate; a.min_cutoff = min_cutoff; a.beta = beta; a.d_cutoff = d_cutoff; a.t_min_cutoff = trans_min_cutoff; a.t_beta = trans_beta;
  a.s_rot = state_rot; a.s_omega = state_omega; a.s_gap = state_gap; a.s_trans = state_trans; a.s_vel = state_velocity;
  a.s_tgap = state_trans_gap; a.rot_out = rot_out; a.trans_out = trans_out;
  hipLaunchKernelGGL(track_one_euro_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}
