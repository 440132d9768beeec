// Evaluation report (csrc/metrics.hip): what the C entry points in capi.hip need to know about its plan and launches.
#pragma once
#include "common.h"

namespace riggs {

#define MT_LEVELS 6  // five MS-SSIM levels + the piq.ssim level (index 5; level 0 itself when its pooling factor is 1)

// Where everything of one call lives inside the caller's workspace, and the pyramid's sizes.  Depends on (B, C, H, W) only: the
// MS-SSIM levels are planned whenever the image admits them (min side > 160), wanted or not, so that the size query needs no flags.
struct MetricsPlan {
  int f;                       // piq's pooling factor: max(1, round_half_even(min(H, W) / 256))
  int ms;                      // the image admits MS-SSIM (min(H, W) > 160)
  int h[MT_LEVELS], w[MT_LEVELS];            // level sizes (0 where a level does not exist)
  int tx[MT_LEVELS], ty[MT_LEVELS];          // workgroups of the level kernel per plane
  size_t part[MT_LEVELS];      // offset of the level's partial sums, in doubles: [plane][workgroup][4]
  size_t img[MT_LEVELS];       // offset of the level's image pair, in floats: x planes then y planes (levels 1..5)
  size_t total_floats;
};
MetricsPlan metrics_plan(int B, int C, int H, int W);
int launch_image_metrics(const MetricsPlan& p, int B, int C, int H, int W, const float* x, const float* y, int clamp, int want_ms,
                         float* out, float* levels, float* workspace, hipStream_t s);

}  // namespace riggs
