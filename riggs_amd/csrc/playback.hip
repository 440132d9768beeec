// Pose-track playback, the part in front of the skinning (riggs_amd/playback.py): key poses -> a track of interpolated poses.
//   slerp_batch        skeleton_utils/interpolation_utils.py:4-54
//   run_interpolation  skeleton_utils/interpolation_utils.py:58-86 (every segment, rotations and translations, in one launch)
// Built with FP contraction off: the steps are the reference's, one rounding each.
#include "common.h"

namespace riggs {

struct SlerpArgs {
  int S, m, n;                // segments, frames per segment, quaternions per pose
  const float *q0, *q1;       // segment s reads q0 + s * q_stride and q1 + s * q_stride, (n, 4) each
  const float* t;             // (m,)
  const float *tr0, *tr1;     // segment s reads tr0 + 3 s and tr1 + 3 s; or NULL: no translations
  long long q_stride;         // floats
  long long os, of, on;       // floats between two segments / frames / quaternions of out_rot
  float *out_rot, *out_trans;  // out_trans: (S * m, 3)
};

// one thread per (segment, frame, quaternion); the threads of quaternion 0 also interpolate the frame's translation
__global__ __launch_bounds__(256) void pose_slerp_kernel(SlerpArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.S * a.m * a.n) return;
  const int j = (int)(i % a.n);
  const int f = (int)((i / a.n) % a.m);
  const int s = (int)(i / ((long long)a.n * a.m));
  const float* p0 = a.q0 + s * a.q_stride + 4 * j;
  const float* p1 = a.q1 + s * a.q_stride + 4 * j;
  float u[4], v[4];
  // :20-21 unit quaternions
  const float n0 = sqrtf(((p0[0] * p0[0] + p0[1] * p0[1]) + p0[2] * p0[2]) + p0[3] * p0[3]);
  const float n1 = sqrtf(((p1[0] * p1[0] + p1[1] * p1[1]) + p1[2] * p1[2]) + p1[3] * p1[3]);
#pragma unroll
  for (int e = 0; e < 4; e++) { u[e] = p0[e] / n0; v[e] = p1[e] / n1; }
  // :24-31 the shorter arc, the clamp
  float dot = ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) + u[3] * v[3];
  if (dot < 0.0f) {
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = -v[e];
  }
  dot = fminf(fmaxf(fabsf(dot), -1.0f), 1.0f);
  // :34-48 the weights; linear where sin(theta_0) <= 1e-6 (0 / 0 of an identical pair never leaves the other branch)
  const float th = acosf(dot), sn = sinf(th), t = a.t[f];
  float w0 = 1.0f - t, w1 = t;
  if (sn > 1e-6f) {
    w0 = sinf((1.0f - t) * th) / sn;
    w1 = sinf(t * th) / sn;
  }
  // :51-54
  float r[4];
#pragma unroll
  for (int e = 0; e < 4; e++) r[e] = w0 * u[e] + w1 * v[e];
  const float nr = sqrtf(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);
  float* o = a.out_rot + s * a.os + f * a.of + j * a.on;
#pragma unroll
  for (int e = 0; e < 4; e++) o[e] = r[e] / nr;
  if (j == 0 && a.tr0) {  // :75-76
    const float* t0 = a.tr0 + 3 * s;
    const float* t1 = a.tr1 + 3 * s;
    float* ot = a.out_trans + 3 * ((long long)s * a.m + f);
#pragma unroll
    for (int e = 0; e < 3; e++) ot[e] = (1.0f - t) * t0[e] + t * t1[e];
  }
}

}  // namespace riggs

using namespace riggs;

extern "C" int riggs_pose_slerp(int32_t num_segments, int32_t num_frames, int32_t num_quats, const float* q0, const float* q1,
                                int64_t q_stride, const float* t, const float* trans0, const float* trans1,
                                int64_t out_stride_segment, int64_t out_stride_frame, int64_t out_stride_quat, float* out_rot,
                                float* out_trans, riggs_stream stream) {
  RIGGS_REQUIRE(num_segments >= 0 && num_frames >= 0 && num_quats >= 0, "riggs_pose_slerp: negative count");
  RIGGS_REQUIRE((trans0 == nullptr) == (trans1 == nullptr) && (trans0 == nullptr || out_trans != nullptr),
                "riggs_pose_slerp: translations come as trans0, trans1 and out_trans, or not at all");
  const long long total = (long long)num_segments * num_frames * num_quats;
  if (total == 0) return 0;
  RIGGS_REQUIRE(q0 && q1 && t && out_rot, "riggs_pose_slerp: q0, q1, t and out_rot are required");
  RIGGS_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "riggs_pose_slerp: too many quaternions");
  SlerpArgs a;
  a.S = num_segments; a.m = num_frames; a.n = num_quats; a.q0 = q0; a.q1 = q1; a.t = t; a.tr0 = trans0; a.tr1 = trans1;
  a.q_stride = q_stride; a.os = out_stride_segment; a.of = out_stride_frame; a.on = out_stride_quat;
  a.out_rot = out_rot; a.out_trans = out_trans;
  hipLaunchKernelGGL(pose_slerp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  RIGGS_HIP_CHECK(hipGetLastError());
  return 0;
}
