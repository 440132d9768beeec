/*
 * riggs_hip.h — C ABI of libriggs_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for RigGS's per-frame hot path.  Every entry point names the
 * reference interface it replaces (paths relative to the RigGS tree).  Plain
 * pointers and sizes only: all `const float*` / `float*` arguments are DEVICE
 * pointers (HBM) unless stated, `stream` is a hipStream_t, nothing here owns
 * memory — the caller (PyTorch's caching allocator, or any hipMalloc) does.
 * Every function returns 0 on success, non-zero on error (see riggs_last_error()).
 *
 * Binding stubs for the reference side are shown in INTEGRATION.md.
 */
#ifndef RIGGS_HIP_H
#define RIGGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* riggs_stream; /* hipStream_t */

/* The ABI version.  It is bumped when the signature of an EXISTING function or the layout of an EXISTING struct changes; added
 * symbols and enumerators appended to an enum do not bump it (the ABI grows: a caller that needs a new symbol resolves it by
 * name; nor does a REMOVED symbol or option name: a consumer that still names it fails at symbol resolution, or with "unknown
 * option").  riggs_version() returns the value the library was built with; a consumer compiled against this header compares that
 * with its own RIGGS_ABI_VERSION and refuses the library when they differ (riggs_amd/_lib.py, csrc_torch/riggs_torch.cpp). */
#define RIGGS_ABI_VERSION 102
int riggs_version(void);
const char* riggs_last_error(void);

/* Library options (process-wide; the library reads NOTHING from the environment).  Names and defaults:
 *   "fwd_wide_tiles"    256   at most this many tiles per frame are composited by the forward's 32-lanes-per-pixel blocks (0 = none)
 *   "fwd_wide_min"      4096  ... the tiles whose walk went this many instances deep in the previous frame of the same arena
 *                             and whose list is that long now (minimum 256; a negative value restores the default)
 *   "fwd_hist_view_tol" 20    ... in the last frame of the SAME VIEW: the arena keeps 128 walk histories, each with the view matrix of its
 *                             frames; a frame uses (and updates) the one no entry of whose matrix is further than value / 100 from
 *                             cfg.viewmatrix, or starts a new one (round robin).  0 = one history whatever the view
 *   "bin_grouped"       -1    which tile sort riggs_raster_render runs where both fit: -1 = chosen by the number of Gaussians
 *                             and of tiles, 0 = the direct counting sort, 1 = the two-level sort (identical lists, bit for bit).
 *                             riggs_raster_binning_bytes reserves the larger of the two layouts, so flipping this never
 *                             invalidates an arena
 *   "color_side_jobs"   1     the SH colours of a frame are evaluated by extra workgroups of the tile sort's scatter launch
 *                             (riggs_raster_render) wherever the direct tile sort runs, instead of by riggs_raster_preprocess's
 *                             kernel: the same colours and clamp bits, bit for bit; the geometry arena's colours are then
 *                             complete after riggs_raster_render, not after riggs_raster_preprocess.  0 = always in preprocess.
 *                             Like "bin_grouped", it must not change between the two calls of one frame
 *   "preprocess_bwd_lean" -1  riggs_raster_backward's per-Gaussian kernel as one wave per 256 Gaussians (no LDS image, every block
 *                             resident at once): -1 = with cfg.sparse_zero (sparse gradient rows: -3 .. -6 us of a frame; with
 *                             every row written the 256-thread form is 18 us faster), 0 / 1 = never / always.  Same results
 *   "pose_mlp_layered"  0     1 = riggs_pose_mlp_forward / _backward(_fk) run one launch per layer (no workgroup hand-off inside a
 *                             launch, nothing that can time out; ~20 launches instead of 2) whatever the network's size: what a
 *                             host re-runs a frame with after the one-launch kernels reported a lost hand-off.  It must not
 *                             change between the forward and the backward of one frame
 *   "rays_reread"       0     riggs_fit_rays keeps a joint's rays in registers for all iterations (0) or reads them from
 *                             global memory again in every iteration (1): the same operations, the same bits (NOTES.md has
 *                             the measurement behind the default)
 * Unknown names fail.  Set them between frames, not while a launch that reads them is being issued from another thread. */
int riggs_set_option(const char* name, int32_t value);
int riggs_get_option(const char* name, int32_t* value);

/* =====================================================================
 * Rasterizer.  Replaces the un-vendored CUDA extension
 *   diff_gaussian_rasterization._C.rasterize_gaussians / rasterize_gaussians_backward
 * reached from gaussian_renderer/__init__.py:14,57-72 (settings) and :133-141 (call).
 * ===================================================================== */

/* Mirror of GaussianRasterizationSettings (gaussian_renderer/__init__.py:57-70).
 * bg / viewmatrix / projmatrix / campos are device tensors exactly as render() builds them
 * (4x4 matrices in the transposed row-vector convention of scene/cameras.py:61-71). */
typedef struct riggs_raster_cfg {
  int32_t num_points;     /* N */
  int32_t sh_degree;      /* active degree 0..3 */
  int32_t sh_coeffs;      /* M = shs.shape[1] (16 for max degree 3); 0 with colors_precomp */
  int32_t image_height;
  int32_t image_width;
  float tanfovx;
  float tanfovy;
  float scale_modifier;
  const float* bg;         /* (3,) */
  const float* viewmatrix; /* (4,4) */
  const float* projmatrix; /* (4,4) */
  const float* campos;     /* (3,) */
  int32_t debug;           /* pipe.debug: synchronise + validate after each stage */
  /* Fused "render glue" (gaussian_renderer/__init__.py:74-92, scene/gaussian_model.py:104-132):
   * when glue != 0 the rasterizer takes RAW parameters and applies
   *   means3D = xyz + d_xyz, opacity = sigmoid(_opacity), scales = exp(_scaling) + d_scaling,
   *   rotations = normalize(_rotation + d_rotation)
   * in-kernel, and the backward returns gradients w.r.t. the raw tensors. */
  int32_t glue;
  int32_t isotropic;       /* glue only: _scaling is (N,1) repeated (gaussian_model.py:105-108) */
  /* Ordered-reduction mode of the compositing backward ("deterministic-reduction mode for grads"): instead of
   * float atomics into the per-Gaussian accumulators, every (tile instance) writes its partial gradient row and a second
   * kernel sums each Gaussian's rows in ascending tile order: gradients are bitwise reproducible run to run.  Needs the
   * larger workspace of riggs_raster_backward_workspace_bytes_ordered; slower (tests / debugging).
   * riggs_raster_render: with it the forward never uses the previous frame's walk history, so it is bitwise reproducible
   * frame after frame; without it the forward is bitwise reproducible only while no tile is composited wide — always in a
   * fresh (zero-filled) binning arena — because a tile composited by the 32-lane blocks folds its sums in another order
   * (same values to ~1e-7; "fwd_wide_tiles" = 0 turns that off as well). */
  int32_t deterministic;
  /* riggs_raster_backward only.  1 = the caller guarantees that the gradient output buffers are the SAME buffers the previous
   * riggs_raster_backward with this workspace wrote and that nobody has written them since (or that buffers and workspace
   * were zero-filled together): rows that receive no gradient now and received none then are not rewritten — they still
   * hold their zeros.  The zero fill of those rows (86-93 % of them per frame) is two thirds of the per-Gaussian backward's
   * HBM traffic.  A captured frame with static gradient buffers qualifies (riggs_amd.graph.GraphedFrame); an eager
   * autograd backward, whose outputs are fresh allocations, does not.  riggs_grad_rows_unpack keeps the guarantee intact
   * when it is given the workspace (it records the rows it writes). */
  int32_t sparse_zero;
  /* 1 = tight instance lists: a Gaussian's tile rectangle (upstream: every tile its ceil(3 sigma) square overlaps) is cut down
   * to the tiles in which alpha = o * exp(power) can reach 1/255 at some pixel centre, by the axis-aligned box of that
   * region (conservative margins).  The dropped instances contribute nothing to any pixel or gradient — they fail the
   * alpha test at every pixel of their tile — so images and gradients are the canonical ones to rounding (the lists'
   * positions move, and with them the grouping of the transmittance products); `radii` is unchanged; the instance list is
   * the canonical list with those instances removed, in the same order.  About a fifth of the instances of a translucent
   * scene (tools/dead_instances.py); the canonical lists (0) are the default and what the ordering parity tests pin. */
  int32_t tight_lists;
} riggs_raster_cfg;

/* Opaque arenas (upstream: geomBuffer / binningBuffer / imgBuffer byte tensors).  The binning arena's size depends on ALL
 * four arguments (the tile sort's tables are sized by the number of Gaussians and of tiles, not only by the instance
 * capacity) and is NOT monotonic in them in general: ask again whenever num_points, image_height or image_width change
 * (in either direction), and pass the arena's byte size to riggs_raster_render, which rejects an arena that is too small
 * for its arguments.  A freshly allocated binning arena must be zero-filled once (its walk-history stamp). */
size_t riggs_raster_geom_bytes(int32_t num_points);
size_t riggs_raster_image_bytes(int32_t image_height, int32_t image_width);
size_t riggs_raster_binning_bytes(int64_t instance_capacity, int32_t num_points, int32_t image_height,
                                  int32_t image_width);
/* The binning arena carries ONE piece of state from frame to frame: how deep the forward walked every tile's list (which
 * tiles the next frame composites with 32 lanes per pixel), kept PER VIEW (128 histories, each with the view matrix of its
 * frames: "fwd_hist_view_tol"), valid when a stamp word derived from the tile and Gaussian counts follows it.  Call this after allocating an arena and whenever (capacity, N, H, W) change for an arena in use
 * (the words' offset depends on them): the next frame then starts without a history.  Equivalent: zero-fill the arena. */
int riggs_raster_binning_reset_history(void* binning, int64_t instance_capacity, int32_t num_points, int32_t image_height,
                                       int32_t image_width, riggs_stream stream);

/* Field offsets (bytes) inside the arenas, for tests / debugging tools. */
enum {
  RIGGS_GEOM_XYD = 0,      /* float4 (px, py, depth, x half extent of the alpha >= 1/255 box) */
  RIGGS_GEOM_CONIC_O,      /* float4 (A, B, C, opacity) */
  RIGGS_GEOM_RGB,          /* float4 (r, g, b, y half extent of that box); complete after riggs_raster_render ("color_side_jobs") */
  RIGGS_GEOM_COV3D,        /* float[6] */
  RIGGS_GEOM_CLAMPED,      /* uint8 bitmask (bit ch) */
  RIGGS_GEOM_TILES,        /* uint32 tiles_touched */
  RIGGS_GEOM_RECT,         /* ushort4 (x0, y0, x1, y1) */
  RIGGS_GEOM_DEPTH_ORDER,  /* uint32: Gaussian indices sorted by depth bits */
  RIGGS_GEOM_NFIELDS_
};
enum {
  RIGGS_IMG_FINAL_T = 0,   /* float  H*W */
  RIGGS_IMG_N_CONTRIB,     /* uint32 H*W */
  RIGGS_IMG_RANGES,        /* uint2  tiles */
  RIGGS_IMG_FWD_CTR,       /* uint32[3] of the last forward: non-empty tiles, tiles composited by the 32-lane blocks, empty tiles */
  RIGGS_IMG_NFIELDS_
};
enum {
  RIGGS_BIN_POINT_LIST = 0, /* uint32 [capacity]: Gaussian index per sorted instance */
  RIGGS_BIN_TILE_KEYS,      /* uint32 [capacity]: tile id per sorted instance (written with cfg.debug only) */
  RIGGS_BIN_WALK_HIST,      /* uint32: the forward's walk histories, one per view — [0] round-robin cursor, [1] the slot of the last frame,
                               [16 ..] 128 slots of ((tiles + 18) rounded up to 16) words: depths per tile, a stamp, the view matrix */
  RIGGS_BIN_NFIELDS_
};
int riggs_raster_geom_layout(int32_t num_points, size_t* offsets /*[RIGGS_GEOM_NFIELDS_]*/);
int riggs_raster_image_layout(int32_t image_height, int32_t image_width, size_t* offsets /*[RIGGS_IMG_NFIELDS_]*/);
int riggs_raster_binning_layout(int64_t instance_capacity, int32_t num_points, int32_t image_height,
                                int32_t image_width, size_t* offsets /*[RIGGS_BIN_NFIELDS_]*/);

/* Stage 1 (per Gaussian): projection, covariance, SH colour, tile rectangle; then the
 * depth sort of the Gaussians and the scan of tiles_touched.  Writes the number of tile
 * instances R into counters[0] (device).  Inputs follow GaussianRasterizer.forward
 * (gaussian_renderer/__init__.py:133-141): exactly one of shs / colors_precomp and exactly
 * one of (scales, rotations) / cov3D_precomp is non-NULL.
 * With cfg->glue: means3D=_xyz, opacities=_opacity(logit), scales=_scaling(log), rotations=_rotation,
 * and d_xyz (N,3) / d_rotation (N,4) / d_scaling (N,3) may be NULL (treated as 0, the Python-float case;
 * scales = exp(_scaling) + d_scaling as at gaussian_renderer/__init__.py:89). */
int riggs_raster_preprocess(const riggs_raster_cfg* cfg, const float* means3D, const float* shs,
                            const float* shs_rest /* NULL, or (N,M-1,3) with shs = (N,1,3): the reference's
                            _features_dc / _features_rest pair read in place, no torch.cat */,
                            const float* colors_precomp, const float* opacities, const float* scales,
                            const float* rotations, const float* cov3D_precomp, const float* d_xyz,
                            const float* d_rotation, const float* d_scaling, void* geom, int32_t* radii,
                            uint32_t* counters /* device [4]: R, overflow, rsv, rsv */, riggs_stream stream);

/* Stage 2: stable counting sort of the (depth-ordered) Gaussians' tile instances by tile — the order of upstream's
 * duplicateWithKeys + 64-bit key sort + identifyTileRanges — and the per-tile alpha compositing.
 * Limits: at most 65 535 tiles and ~4 200 groups of eight tiles in a row (3840 x 2160 px is fine): beyond 25 600 tiles, and
 * from 500 000 Gaussians over 4 096 tiles on, the sort runs in two levels (by tile group, then by tile; the same list bit
 * for bit; riggs_set_option("bin_grouped", 0 / 1) forces the choice where both fit) — larger images are rejected with an
 * error, never mis-rendered.  `instance_capacity` bounds R: if R > capacity the launch is
 * still memory-safe, counters[1] is set to 1 and the image is undefined (caller retries
 * with a larger arena; riggs_amd.rasterizer does that). */
int riggs_raster_render(const riggs_raster_cfg* cfg, const void* geom, void* binning, int64_t instance_capacity,
                        size_t binning_bytes /* size of `binning`: must be >= riggs_raster_binning_bytes(capacity, N, H, W) */,
                        void* image_state, float* out_color /*(3,H,W)*/, float* out_depth /*(1,H,W)*/,
                        float* out_alpha /*(1,H,W)*/, uint32_t* counters, riggs_stream stream);

/* Backward of both stages.  Gradient outputs are fully written (no pre-zeroing needed).
 * `counters` is the forward's: when its overflow flag (counters[1]) is set the frame composited truncated
 * lists, and the backward writes exact ZERO gradients (device-side guard: an optimizer step queued behind it —
 * e.g. inside a captured hipGraph — sees zeros, never garbage); NULL skips the guard.
 * dL_ddepth / dL_dalpha may be NULL (RigGS stage 2 uses only "render": train_rig.py:499).
 * Outputs that do not apply (e.g. dL_dsh with colors_precomp) may be NULL.
 * With cfg->glue the outputs are gradients w.r.t. the raw tensors: dL_dmeans3D = dL/d_xyz = dL/dd_xyz,
 * dL_dopacities = dL/d_opacity(logit), dL_dscales = dL/d_scaling(log; (N,1) when isotropic),
 * dL_drotations = dL/d_rotation = dL/dd_rotation. */
int riggs_raster_backward(const riggs_raster_cfg* cfg, const float* means3D, const float* shs,
                          const float* shs_rest, const float* colors_precomp, const float* opacities, const float* scales,
                          const float* rotations, const float* cov3D_precomp, const float* d_xyz,
                          const float* d_rotation, const float* d_scaling, const int32_t* radii, const void* geom, const void* binning,
                          int64_t instance_capacity, const void* image_state, const uint32_t* counters,
                          const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                          void* workspace /* riggs_raster_backward_workspace_bytes(N); must be ALL ZERO on first use; the
                          accumulators in it are all zero again on return (self-cleaning): zero it once after allocating and
                          keep it — for THIS num_points: behind the accumulators the call leaves one bit per Gaussian "received a gradient"
                          (riggs_grad_rows_*), at an offset that depends on num_points; re-zero the buffer before another size uses it */,
                          float* dL_dmeans3D,
                          float* dL_dmeans2D /*(N,3)*/, float* dL_dsh, float* dL_dcolors_precomp,
                          float* dL_dopacities, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                          float* dL_dd_scaling /* glue only, may be NULL */,
                          float* dL_dsh_rest /* with shs_rest: (N,M-1,3), dL_dsh is then (N,1,3) */,
                          riggs_stream stream);
size_t riggs_raster_backward_workspace_bytes(int32_t num_points);
/* where the workspace keeps its row list (one bit per Gaussian: "holds a gradient"): a caller that has written the gradient
 * buffers itself (e.g. a dense all-reduce in place) fills these bytes with 0xFF before the next backward with
 * cfg.sparse_zero, which then rewrites every row */
int riggs_raster_backward_workspace_rows(int32_t num_points, size_t* offset, size_t* bytes);
/* cfg->deterministic: [accumulators | one row of 10 floats per tile instance | the instances of every Gaussian in tile order |
 * their offsets]; need not be zeroed */
size_t riggs_raster_backward_workspace_bytes_ordered(int32_t num_points, int64_t instance_capacity);

/* A second colour set over a rendered frame's tile lists.  Replaces the SECOND render() of the same camera and geometry that
 * differs only in the per-Gaussian colour: the motion-mask render of train_gui.py:1123-1130 (render_motion=True, every geometry
 * input detached, colours [m, 0, 1-m]: gaussian_renderer/__init__.py:94-98), render_rig.py:152-160 (override_color=skinning_color).
 * `geom`, `binning`, `image_state`, `counters` are those of a frame after riggs_raster_render — all READ ONLY here, so the frame's
 * own riggs_raster_backward may run before or after; cfg gives num_points, image_height, image_width (and debug), the rest of it is
 * not read.  No preprocess, no sort, no binning: per pixel
 *   out[ch] = sum_i colors[i][ch] alpha_i T_i + final_T bg[ch]
 * over the instances of the pixel's tile list in front of its n_contrib — the set the frame's forward composited —, with the alpha
 * evaluation of the compositing backward.  `bg` is this call's own and need not be the frame's.
 * The backward is the colour gradient only, dL/dcolors[n][ch] = sum_pix alpha T dL_dcolor[ch][pix] (float atomics, one triple per
 * contributing (instance, tile)); it zero-fills dL_dcolors itself on the stream, so the buffer is fully written.
 * counters != NULL: when the frame's overflow flag (counters[1]) is set the forward writes a ZERO image and the backward ZERO
 * gradients, decided on the device (as riggs_raster_backward); NULL skips the guard.  num_points == 0 is valid: the image is bg.
 * Neither call allocates, reads back or synchronises (cfg.debug: synchronises and checks): both are legal inside a stream capture.
 * (Added symbols: RIGGS_ABI_VERSION is unchanged.) */
int riggs_raster_recolor_forward(const riggs_raster_cfg* cfg /* N, H, W */, const void* geom, const void* binning,
                                 int64_t instance_capacity, const void* image_state, const uint32_t* counters /* NULL: no guard */,
                                 const float* colors /*(N,3)*/, const float* bg /*(3,)*/, float* out_color /*(3,H,W)*/,
                                 riggs_stream stream);
int riggs_raster_recolor_backward(const riggs_raster_cfg* cfg, const void* geom, const void* binning, int64_t instance_capacity,
                                  const void* image_state, const uint32_t* counters, const float* dL_dcolor /*(3,H,W)*/,
                                  float* dL_dcolors /*(N,3), fully written*/, riggs_stream stream);

/* =====================================================================
 * Skeleton deformation.  Replaces the torch-op graph of
 *   SkeletonWarp.deform_by_pose  skeleton_utils/skeleton_warp.py:130-172
 * ===================================================================== */

/* Forward kinematics + helpers on ONE workgroup:
 *   quaternion_to_matrix      utils/time_utils.py:115-132
 *   chain_product_transform   skeleton_utils/skeleton_warp.py:242-273
 *   matrix_to_quaternion      utils/time_utils.py:146-205 (on the detached global rotations)
 * local_rot (J,4) un-normalised wxyz; joints (J,3); parents (J,) int32 with parents[i] < i; 1 <= J <= 256 (J <= 64: one
 * wave64, 65..256: one 256-thread workgroup, a barrier per tree level).
 * Outputs: transforms (J,12) = rows of [R|t] 3x4, node_rot (J,4), d_nodes (J,3) = posed + global_trans. */
int riggs_fk_forward(int32_t num_joints, const float* local_rot, const float* joints, const int32_t* parents,
                     const float* global_trans, float* transforms, float* node_rot, float* d_nodes,
                     riggs_stream stream);
/* Reverse sweep: (dL/dtransforms (J,12), dL/dd_nodes (J,3) or NULL) -> dL/dlocal_rot (J,4);
 * accumulates sum_j dL/dd_nodes into dL_dglobal_trans (3) (+=). */
int riggs_fk_backward(int32_t num_joints, const float* local_rot, const float* joints, const int32_t* parents,
                      const float* dL_dtransforms, const float* dL_dd_nodes, float* dL_dlocal_rot,
                      float* dL_dglobal_trans, riggs_stream stream);

/* Bone-distance skinning weights + linear blend skinning, fused:
 *   cal_nn_weight_skeleton        skeleton_warp.py:41-76   (gs_kernel, K = -1 or top-K)
 *   line_segment_distance         skeleton_warp.py:215-238 (squared)
 *   LBS of means / quaternion     skeleton_warp.py:149-165
 * x (N,3), motion_mask (N,) or NULL (= ones), node_radius_log (J,) = SkeletonWarp._node_radius.
 * Outputs d_xyz (N,3), d_rotation (N,4); optional nn_weight (N,Kp) / nn_idx (N,Kp) int64 where
 * Kp = J-1 (K<=0) or K — needed by render_rig.py:156-158, not by training (may be NULL).  2 <= J <= 256 (J > 64: kernels of
 * their own with up to 255 bone records in LDS; riggs_lbs_forward_fk then runs the chain as a launch in front). */
int riggs_lbs_forward(int32_t num_points, int32_t num_joints, int32_t K, const float* x, const float* joints,
                      const int32_t* parents, const float* node_radius_log, const float* transforms,
                      const float* node_rot, const float* global_trans, const float* motion_mask,
                      const float* weight_mod /* NULL, or (N, J-1) = sigmoid(WeightMLP(x)): skeleton_warp.py:56-69; K = -1 only */,
                      float* d_xyz, float* d_rotation, float* nn_weight, int64_t* nn_idx,
                      void* bone_table /* may be NULL; riggs_lbs_bone_table_bytes() of device scratch, see below */,
                      riggs_stream stream);
/* bone_table (riggs_lbs_forward / riggs_lbs_forward_fk; may be NULL): device scratch of riggs_lbs_bone_table_bytes() bytes.  Given
 * one, a forward over <= 64 joints always leaves its staged bone records there (segment, radius term, transform and rotation of
 * every bone), whichever kernel runs: riggs_lbs_backward_table stages from them instead of building them again in every
 * workgroup.  Results are bit-identical with and without a table, forward and backward.  Also, with
 * it the all-bones forward (K = -1, no weight_mod, no nn outputs) of a LARGE scene (>= 1 M Gaussians, >= 16 joints) reads the bone
 * records through the scalar cache as SGPR operands — a one-workgroup launch writes the table (and, in the _fk form, runs the
 * chain) in front — instead of staging them in every workgroup's LDS: 2 M x 64 joints 129 -> 104 us, results bit-identical.
 * riggs_set_option("lbs_scalar", 1 / -1) forces / forbids the form at every size (default 0: by size).  A <= 64-joint form: the
 * table holds 64 records, and skeletons of more joints never read it. */
size_t riggs_lbs_bone_table_bytes(void);
/* The same with the forward kinematics INSIDE the launch (every workgroup runs the chain of J - 1 dependent 3x4 products
 * itself — 2 us — instead of a launch of its own in front — 6.5 us of a captured frame): takes the pose, and workgroup 0
 * leaves what riggs_fk_forward would have written (transforms (J,12), node_rot (J,4), d_nodes (J,3)) for the backward and
 * the caller.  SkeletonWarp.forward(x, t, mask) uses it (riggs_amd/skeleton.py: _PoseDeform). */
int riggs_lbs_forward_fk(int32_t num_points, int32_t num_joints, int32_t K, const float* x, const float* joints,
                         const int32_t* parents, const float* node_radius_log, const float* local_rot,
                         const float* global_trans, const float* motion_mask, const float* weight_mod,
                         float* transforms, float* node_rot, float* d_nodes, float* d_xyz, float* d_rotation,
                         void* bone_table, riggs_stream stream);
/* Backward: cotangents g_xyz (N,3), g_rot (N,4) -> dL/dtransforms (J,12), dL/dnode_radius_log (J),
 * dL/dglobal_trans (3), optional dL/dmotion_mask (N).  Reduction over N is done in-kernel
 * (registers -> workgroup partials -> a fixed-order second stage: run-to-run deterministic).
 * No gradient to x or joints (both detached in the reference: skeleton_warp.py:16,44,131). */
int riggs_lbs_backward(int32_t num_points, int32_t num_joints, int32_t K, const float* x, const float* joints,
                       const int32_t* parents, const float* node_radius_log, const float* transforms,
                       const float* node_rot, const float* global_trans, const float* motion_mask,
                       const float* weight_mod, const float* g_xyz, const float* g_rot, float* dL_dtransforms,
                       float* dL_dnode_radius_log, float* dL_dglobal_trans, float* dL_dmotion_mask,
                       float* dL_dweight_mod /* (N, J-1), required with weight_mod */,
                       void* workspace /* riggs_lbs_backward_workspace_bytes(N, J) */, riggs_stream stream);
size_t riggs_lbs_backward_workspace_bytes(int32_t num_points, int32_t num_joints);
/* The same backward with the bone table that the forward of the SAME inputs (joints, parents, node_radius_log, transforms,
 * node_rot) filled: every workgroup copies the records with one coalesced read where riggs_lbs_backward rebuilds them (per bone
 * two dependent loads, an exp and two divisions, in front of the walk).  bone_table NULL, or more than 64 joints: exactly
 * riggs_lbs_backward.  Gradients are bit-identical to it wherever it is reproducible itself.  The table lives with what the
 * forward saves for the backward and is read only.  (Added symbol: RIGGS_ABI_VERSION is unchanged.) */
int riggs_lbs_backward_table(int32_t num_points, int32_t num_joints, int32_t K, const float* x, const float* joints,
                             const int32_t* parents, const float* node_radius_log, const float* transforms,
                             const float* node_rot, const float* global_trans, const float* motion_mask,
                             const float* weight_mod, const float* g_xyz, const float* g_rot, float* dL_dtransforms,
                             float* dL_dnode_radius_log, float* dL_dglobal_trans, float* dL_dmotion_mask,
                             float* dL_dweight_mod, const void* bone_table /* may be NULL */,
                             void* workspace /* riggs_lbs_backward_workspace_bytes(N, J) */, riggs_stream stream);

/* ---- Playback of a pose track (inference only: no backward exists; riggs_amd/playback.py).  Added symbols: RIGGS_ABI_VERSION
 * is unchanged.
 * riggs_lbs_sequence_forward: M poses over ONE canonical cloud.  A launch in front runs the kinematic chain of every frame
 * (one wave per frame up to 64 joints, one 256-thread workgroup beyond) and writes transforms (M,J,12), node_rot (M,J,4),
 * d_nodes (M,J,3); the skinning launch keeps one Gaussian per thread — position, top-K set, weight_mod row: once — and walks
 * the track in passes of riggs_lbs_sequence_pass_frames(J, K) frames whose (G, q) records lie in LDS, a bone's weight evaluated
 * once per pass.  local_rot (M,J,4); global_trans (M,3) with global_trans_stride = 3, or (3,) with 0; motion_mask (N,) or NULL;
 * weight_mod (N,J-1) or NULL (K = -1 only).  Outputs d_xyz (M,N,3), d_rotation (M,N,4): frame-major, a frame is contiguous.
 * Same weights as riggs_lbs_forward (shared code), 2 <= J <= 256. */
int riggs_lbs_sequence_forward(int32_t num_points, int32_t num_frames, int32_t num_joints, int32_t K, const float* x,
                               const float* joints, const int32_t* parents, const float* node_radius_log, const float* local_rot,
                               const float* global_trans, int32_t global_trans_stride, const float* motion_mask,
                               const float* weight_mod, float* transforms, float* node_rot, float* d_nodes, float* d_xyz,
                               float* d_rotation, riggs_stream stream);
int32_t riggs_lbs_sequence_pass_frames(int32_t num_joints, int32_t K);
/* The skinning weights of riggs_lbs_forward folded into one colour per Gaussian, without nn_weight / nn_idx in memory
 * (skeleton_utils/visualization.py:118-129).  node_colors (J,3): bone k carries the colour of its child joint k + 1.
 * mode 0: sum_k w_k colour; mode 1: the colour of the largest weight (the first such bone on equality), copied unchanged. */
int riggs_skinning_colors(int32_t num_points, int32_t num_joints, int32_t K, const float* x, const float* joints,
                          const int32_t* parents, const float* node_radius_log, const float* weight_mod /* or NULL */,
                          const float* node_colors, int32_t mode, float* colors /* (N,3) */, riggs_stream stream);
/* slerp_batch / run_interpolation (skeleton_utils/interpolation_utils.py:4-86) in one launch: for segment s < num_segments,
 * frame f < num_frames and quaternion j < num_quats, out_rot[s * out_stride_segment + f * out_stride_frame + j * out_stride_quat
 * .. + 4] = slerp(q0[s * q_stride + 4 j ..], q1[s * q_stride + 4 j ..], t[f]) (inputs need not be unit; strides in floats), and —
 * unless trans0 is NULL — out_trans[(s * num_frames + f) * 3 ..] = (1 - t[f]) trans0[3 s ..] + t[f] trans1[3 s ..]. */
int riggs_pose_slerp(int32_t num_segments, int32_t num_frames, int32_t num_quats, const float* q0, const float* q1,
                     int64_t q_stride, const float* t, const float* trans0, const float* trans1, int64_t out_stride_segment,
                     int64_t out_stride_frame, int64_t out_stride_quat, float* out_rot, float* out_trans, riggs_stream stream);

/* =====================================================================
 * PoseMLP (time -> J quaternions + root translation), batch of ONE row:
 *   PoseMLP.forward   skeleton_utils/network_utils.py:134-150  (8 x Linear(256) + ReLU, the
 *   embedding re-concatenated IN FRONT of h after layer `skip`, two linear heads) with the
 *   embedding of utils/time_utils.py:208-256 for input_dims = 1.
 * weights[l] / biases[l] are HOST arrays of `depth` DEVICE pointers to torch's nn.Linear tensors
 * (row-major (out, in)).  `acts` (riggs_pose_mlp_acts_floats floats) is written by forward and
 * read by backward (which also uses its tail — zeroed by forward — for its own hand-off state).  backward writes every parameter gradient into ONE flat buffer laid out as
 *   [W_0, b_0, ..., W_{depth-1}, b_{depth-1}, W_rot, b_rot, W_tr, b_tr]   (no gradient to t).
 * sync_state (may be NULL): riggs_pose_mlp_sync_bytes bytes of device memory, ZEROED ONCE by the caller
 * and then owned by this network (one launch in flight at a time): the forward runs as one launch whose
 * workgroups hand the layer outputs to each other through it, and a generation counter inside makes
 * every launch's tags unique.  With NULL a private copy inside `acts` is cleared by a memset node per call.
 * rot_bias4 (4 floats, may be NULL) is added to every predicted quaternion: the identity bias
 * [1,0,0,0] of skeleton_warp.py:118 folded into the head instead of a separate elementwise op.
 * skip: -1 (none) .. depth - 1.  With skip == depth - 1 the HEADS read [emb, h]: W_rot / W_tr then have width + emb columns
 * (a valid configuration of these entries, tests/test_gpu_pose_mlp_f64.py).  torch's PoseMLP module cannot express it — for
 * depth <= 2 it builds Linear(hidden, ...) heads in front of [emb, h], as the reference does — so riggs_amd.skeleton.PoseMLP keeps
 * such a module on the torch-op path, which raises the reference's own shape error.
 * ===================================================================== */
size_t riggs_pose_mlp_acts_floats(int32_t depth, int32_t width, int32_t multires);
size_t riggs_pose_mlp_sync_bytes(int32_t depth, int32_t width);
/* Index (32-bit words) of the STICKY status word inside sync_state.  The one-launch kernels pass data between
 * workgroups by bounded spinning, which needs all of a launch's workgroups co-resident (<= 96 workgroups of 512
 * threads: true on an otherwise idle MI355X; NOT guaranteed when another process or a concurrent stream holds
 * CUs for long).  A spin that times out poisons that launch's outputs with NaN and sets bit 0 of this word; no
 * kernel ever clears it.  The host reads it after a step (PoseMLP.check_status / GraphedFrame.check) and raises.
 * The word behind it is a TEST HOOK: bit 0 / bit 1 make one workgroup of the forward / backward launch keep a layer's
 * hand-off to itself, so that the time-out path can be exercised on an idle GPU (tests/test_gpu_deform.py); leave it 0. */
size_t riggs_pose_mlp_status_word(int32_t depth, int32_t width);
/* Placement of the one-launch kernels' chain (process-wide; default 1): 1 = its workgroups are every eighth workgroup of the
 * launch, i.e. on ONE XCD when the dispatcher deals round-robin, and hand their layers over through that XCD's L2 (verified
 * inside every launch; falls back by itself when one XCD cannot hold the chain) — 5-7 us faster per launch on an idle device;
 * 0 = the launch's first workgroups, on all XCDs: choose it when another stream keeps compute units busy for long (RCCL
 * collectives overlapped with the deformation backward: the chain needs EVERY compute unit of its XCD to hold one of its
 * workgroups, and waits for the collective's kernel where it cannot).  riggs_amd.dist selects 0 for world sizes > 1. */
int riggs_pose_mlp_set_placement(int32_t one_xcd);
/* debugging aid: 128 device u64 that workgroup 0 of the one-launch kernels stamps with the 100 MHz wall clock
 * per stage (forward [0,64), backward [64,128)); NULL (the default) disables it. */
int riggs_pose_mlp_set_trace(void* dev_u64x128);
size_t riggs_pose_mlp_backward_workspace_floats(int32_t depth, int32_t width, int32_t multires);
int riggs_pose_mlp_forward(int32_t depth, int32_t width, int32_t multires, int32_t skip, int32_t n_rot,
                           const float* const* weights, const float* const* biases, const float* W_rot,
                           const float* b_rot, const float* W_tr, const float* b_tr, const float* t,
                           const float* rot_bias4, void* sync_state, float* acts, float* rotation,
                           float* translation, riggs_stream stream);
int riggs_pose_mlp_backward(int32_t depth, int32_t width, int32_t multires, int32_t skip, int32_t n_rot,
                            const float* const* weights, const float* const* biases, const float* W_rot,
                            const float* b_rot, const float* W_tr, const float* b_tr, float* acts,
                            const float* g_rotation, const float* g_translation, float* workspace,
                            float* flat_grads, void* sync_state /* the forward's, or NULL */, riggs_stream stream);

/* riggs_pose_mlp_backward with the reverse sweep of the kinematic chain (riggs_fk_backward) in front, in the same launch:
 * the gradients of the heads' outputs are computed from (dL/dtransforms (J,12), dL/dd_nodes (J,3) or NULL) by every workgroup
 * of the chain while its weights load, instead of by a launch of one workgroup in front (10 us of a captured frame).
 * g_rotation (4J, may be NULL) is ADDED to the sweep's dL/dlocal_rot (other consumers of the predicted quaternions);
 * g_translation (3, may be NULL) is the gradient of the predicted translation from elsewhere (the skinning's
 * dL/dglobal_trans), to which sum_j dL/dd_nodes_j is added.  dL_dlocal_rot (J,4) and dL_dglobal_trans (3) receive the two
 * totals (required for networks that run one launch per layer, else optional).  n_rot must be 4 * num_joints.
 * template_fixed_coef (device scalar, may be NULL): the template frame's pose regulariser of the stage-2 objective
 * (train_rig.py:474-482: lambda_template_fixed * mean((local_rotation - (1,0,0,0))^2), template camera only) as a cotangent:
 * dL/dlocal_rot += coef * (local_rot - unit), coef = 2 lambda / (4 J) on the template frame and 0 elsewhere, refreshed by the host
 * between replays of a captured iteration; template_fixed_loss (device float, may be NULL) receives mean((local_rot - unit)^2),
 * the value the reference logs.  No launch of its own. */
int riggs_pose_mlp_backward_fk(int32_t depth, int32_t width, int32_t multires, int32_t skip, int32_t n_rot,
                               const float* const* weights, const float* const* biases, const float* W_rot,
                               const float* b_rot, const float* W_tr, const float* b_tr, float* acts, int32_t num_joints,
                               const float* local_rot, const float* joints, const int32_t* parents,
                               const float* transforms /* (J,12) as the forward wrote them, or NULL: the chain is re-run */,
                               const float* dL_dtransforms, const float* dL_dd_nodes, const float* g_rotation,
                               const float* g_translation, float* dL_dlocal_rot, float* dL_dglobal_trans,
                               const float* template_fixed_coef, float* template_fixed_loss, float* workspace,
                               float* flat_grads, void* sync_state, riggs_stream stream);

/* =====================================================================
 * The whole frame behind ONE call per direction — what train_rig.py:535-554 issues per iteration as skeleton.step() + render()
 * + loss.backward(): riggs_pose_mlp_forward -> riggs_lbs_forward_fk -> riggs_raster_preprocess -> riggs_raster_render, and
 * riggs_raster_backward -> riggs_lbs_backward -> riggs_pose_mlp_backward_fk.  Same kernels, same results; the point is the
 * host: an eagerly issued frame crosses the binding seven times and is host-bound (0.65 ms per frame at the bench workload
 * against 0.36 ms of device time); through these two entries it is two crossings.  Every field has the meaning of the
 * like-named argument of the entry points above.  The rasterizer runs with the fused render glue (cfg.glue must be 1): xyz /
 * opacity / scaling / rotation are the RAW parameters, features_dc / features_rest the two SH tensors read in place; `xyz` is
 * also the (detached) input of the skinning.  The binning arena must hold `instance_capacity` instances (a caller that does
 * not know R yet runs its first frame through the separate entry points, as riggs_amd.rasterizer.RasterArena does).
 * ===================================================================== */
typedef struct riggs_frame {
  /* PoseMLP (riggs_pose_mlp_forward) */
  int32_t depth, width, multires, skip, n_rot;
  const float* const* weights; const float* const* biases;       /* host arrays of `depth` device pointers */
  const float *W_rot, *b_rot, *W_tr, *b_tr, *t, *rot_bias4;
  void* sync_state; float* acts;
  float* local_rot;      /* out (J,4) */
  float* global_trans;   /* out (3,) */
  /* skeleton (riggs_lbs_forward_fk) */
  int32_t num_joints, K;
  const float* joints; const int32_t* parents; const float* node_radius_log; const float* motion_mask; const float* weight_mod;
  float *transforms, *node_rot, *d_nodes;   /* out (J,12), (J,4), (J,3) */
  float *d_xyz, *d_rotation;                /* out (N,3), (N,4): the residuals the rasterizer's glue adds */
  /* rasterizer (riggs_raster_preprocess + riggs_raster_render) */
  riggs_raster_cfg cfg;
  const float *xyz, *features_dc, *features_rest, *opacity, *scaling, *rotation, *d_scaling /* or NULL */;
  void* geom; int32_t* radii; uint32_t* counters;
  void* binning; int64_t instance_capacity; size_t binning_bytes; void* image_state;
  float *out_color, *out_depth, *out_alpha;
} riggs_frame;

typedef struct riggs_frame_grads {
  const float *dL_dcolor, *dL_ddepth /* or NULL */, *dL_dalpha /* or NULL */;
  void* raster_workspace;                    /* riggs_raster_backward_workspace_bytes(N), see riggs_raster_backward */
  float *dL_dxyz, *dL_dmeans2D, *dL_dfeatures_dc, *dL_dfeatures_rest, *dL_dopacity, *dL_dscaling, *dL_drotation;
  float* dL_dd_scaling;                      /* or NULL */
  float* dL_dtransforms;                     /* (J,12) scratch: the skinning's gradient, consumed by the chain's reverse sweep */
  float* dL_dnode_radius_log;                /* (J,) */
  float* dL_dglobal_trans_skinning;          /* (3,) scratch */
  float *dL_dmotion_mask, *dL_dweight_mod;   /* or NULL */
  void* lbs_workspace;                       /* riggs_lbs_backward_workspace_bytes(N, J) */
  const float *dL_dd_nodes, *g_local_rot, *g_global_trans; /* cotangents of d_nodes (J,3) / local_rot (J,4) / global_trans (3,)
                                                from other consumers (regularisers, the projection loss), or NULL */
  float *dL_dlocal_rot, *dL_dglobal_trans;   /* out (J,4), (3,) */
  float* pose_workspace;                     /* riggs_pose_mlp_backward_workspace_floats */
  float* pose_flat_grads;                    /* the PoseMLP's parameter gradients, flat, in parameter order */
} riggs_frame_grads;

int riggs_frame_forward(const riggs_frame* frame, riggs_stream stream);
int riggs_frame_backward(const riggs_frame* frame, const riggs_frame_grads* grads, riggs_stream stream);

/* =====================================================================
 * Gaussian optimizer.
 *   GaussianModel.training_setup  scene/gaussian_model.py:197-221 builds torch.optim.Adam(l, lr=0.0, eps=1e-15)
 *   with ONE parameter tensor per group and per-group learning rates; train_rig.py:527 steps it.
 * riggs_adam_step applies that update (plain Adam: no weight decay, no amsgrad; torch's single-tensor
 * operation order) to up to 32 parameter tensors in ONE launch.  All pointer arrays are HOST arrays of
 * DEVICE pointers (16-byte aligned tensors of numel[k] floats); lr[k] is the group's current learning
 * rate, step[k] the step count AFTER this update (>= 1); exp_avg / exp_avg_sq are updated in place.
 *   add_densification_stats       scene/gaussian_model.py:516-518
 *   max_radii2D update            train_rig.py:333-335
 * riggs_densify_stats: for every i with update_filter[i] (bytes, torch.bool layout):
 *   xyz_gradient_accum[i] += ||viewspace_grad[i, :2]||, denom[i] += 1, and if max_radii2D and radii are
 *   non-NULL max_radii2D[i] = max(max_radii2D[i], radii[i]).  viewspace_grad is (N,3).
 * ===================================================================== */
int riggs_adam_step(int32_t n_groups, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const int64_t* numel, const double* lr, const int64_t* step, double beta1,
                    double beta2, double eps, riggs_stream stream);
/* riggs_adam_step for a trainer that issues every call eagerly and never looks at the frame's status words (an unmodified
 * train_rig.py): an element whose gradient is NaN or Inf — what a frame poisoned by a lost PoseMLP hand-off produces — keeps its
 * parameter and both moments, and *nonfinite_count (device u32, not NULL, never reset by the library) is incremented per such
 * element; every other element is updated exactly as by riggs_adam_step.  (The step counts of such a trainer live on the host:
 * a whole-step gate would leave them ahead of the device.  Inside a hipGraph use riggs_adam_step_gated.) */
int riggs_adam_step_guarded(int32_t n_groups, float* const* params, const float* const* grads, float* const* exp_avg,
                            float* const* exp_avg_sq, const int64_t* numel, const double* lr, const int64_t* step, double beta1,
                            double beta2, double eps, uint32_t* nonfinite_count, riggs_stream stream);
/* The same update with the step counts (and optionally the learning rates) in DEVICE memory, the layout of
 * torch.optim.Adam(capturable=True): step_dev[k] / lr_dev[k] are HOST arrays of DEVICE pointers to 0-dim float tensors;
 * step_dev[k][0] holds the count AFTER this update (the caller increments it on the stream beforehand); lr_dev may be
 * NULL or hold NULL entries (then lr[k], a host value baked into the launch, is used).  Safe to capture in a hipGraph. */
int riggs_adam_step_capturable(int32_t n_groups, float* const* params, const float* const* grads, float* const* exp_avg,
                               float* const* exp_avg_sq, const int64_t* numel, const double* lr,
                               const float* const* step_dev, const float* const* lr_dev, double beta1, double beta2,
                               double eps, riggs_stream stream);
/* ---- A frame's "valid" gate.  Every way a frame of this library can go wrong WITHOUT the host noticing in time leaves a
 * non-zero device word behind: the sticky status word of the one-launch PoseMLP kernels (a workgroup hand-off timed out, the
 * pose was poisoned with NaN: sync_state[riggs_pose_mlp_status_word()]), the rasterizer's counters[1] (bit 0: the instance
 * arena overflowed, the lists were truncated; bit 1: the depth sort's in-launch barrier timed out), the gradient-row
 * exchange's status[1] (a segment overflowed or some rank's frame was invalid: nothing was unpacked).  A host that steps its
 * optimizer inside the same hipGraph cannot look at them first — so the kernels that CONSUME a frame's gradients take the
 * words themselves: when (word[i][0] & mask[i]) != 0 for any i < n they leave every output untouched.
 *   riggs_adam_step_gated         = riggs_adam_step_capturable that also advances the step counts (step_dev[k][0] += 1, as a
 *                                   first launch) — parameters, both moments and the counts are bit-identical to before the
 *                                   call when the gate is set, and *skipped (device u32, may be NULL) is incremented instead.
 *   riggs_grad_rows_pack_gated    = riggs_grad_rows_pack that marks the segment "frame invalid" (rows needed = 0xFFFFFFFF)
 *                                   instead of packing: every rank's riggs_grad_rows_unpack then skips (gradients untouched) and
 *                                   raises bit 1 of status[1] — which the ranks' optimizers take as THEIR gate, so that all
 *                                   replicas skip the step together and stay bit-identical.
 *   riggs_gate_flag               writes 1.0f (gate set) or 0.0f into `flag` — a spare float INSIDE the buffer of a dense
 *                                   gradient all-reduce (sum or average), issued in front of that collective: afterwards the
 *                                   slot is non-zero on every rank when SOME rank's frame was invalid (the NaN of a poisoned
 *                                   frame spreads to every rank's gradients through the sum; so does this flag), and serves as
 *                                   a gate word (mask 0x7FFFFFFF) of every rank's optimizer.
 */
#define RIGGS_GATE_MAX 4
typedef struct riggs_gate {
    int32_t n;                                  /* words in use (0: never gated) */
    int32_t reserved;
    const uint32_t* word[RIGGS_GATE_MAX];       /* device pointers */
    uint32_t mask[RIGGS_GATE_MAX];
} riggs_gate;
int riggs_gate_flag(const riggs_gate* gate, float* flag, riggs_stream stream);
/* (advance_steps = 0: the counts were advanced by riggs_adam_steps_advance_gated — one launch for up to 128 of them, what a
 * host with more than 32 parameter tensors issues once in front of its riggs_adam_step_gated calls; `skipped` is counted there) */
int riggs_adam_steps_advance_gated(int32_t n_steps, float* const* step_dev, const riggs_gate* gate, uint32_t* skipped,
                                   riggs_stream stream);
int riggs_adam_step_gated(int32_t n_groups, float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, const int64_t* numel, const double* lr, float* const* step_dev,
                          const float* const* lr_dev, double beta1, double beta2, double eps, const riggs_gate* gate,
                          uint32_t* skipped, int32_t advance_steps, riggs_stream stream);
/* The gated pair with the bias corrections evaluated ONCE: riggs_adam_steps_advance_coef advances the counts like
 * riggs_adam_steps_advance_gated and writes coef[2 k] = 1 - beta1^t, coef[2 k + 1] = sqrt(1 - beta2^t) of the new counts (double
 * precision, one thread per count; coef: 2 n_steps device floats); riggs_adam_step_gated_coef = riggs_adam_step_gated
 * (advance_steps = 0) reading them (coef: the 2 n_groups floats of ITS tensors) instead of evaluating two double-precision pow()
 * in the prologue of each of its 16 384 workgroups — a tenth of the update's time.  All counts of one call share the betas. */
int riggs_adam_steps_advance_coef(int32_t n_steps, float* const* step_dev, const riggs_gate* gate, uint32_t* skipped, double beta1,
                                  double beta2, float* coef, riggs_stream stream);
int riggs_adam_step_gated_coef(int32_t n_groups, float* const* params, const float* const* grads, float* const* exp_avg,
                               float* const* exp_avg_sq, const int64_t* numel, const double* lr, float* const* step_dev,
                               const float* const* lr_dev, double beta1, double beta2, double eps, const riggs_gate* gate,
                               const float* coef, riggs_stream stream);
int riggs_densify_stats(int32_t num_points, const float* viewspace_grad, const uint8_t* update_filter,
                        const int32_t* radii, float* xyz_gradient_accum, float* denom, float* max_radii2D,
                        riggs_stream stream);

/* =====================================================================
 * Gradient-row exchange of the frame-sharded step (the reference is single-GPU:
 * utils/general_utils.py:207 pins cuda:0, so this has no reference counterpart — it is what the data-parallel
 * caller of riggs_raster_backward binds instead of an all-reduce over all N rows).
 * riggs_raster_backward leaves in its workspace which Gaussians received a gradient this frame (the others' gradients
 * are exactly zero in every tensor).  riggs_grad_rows_pack copies those rows — (Gaussian index, row of every tensor in
 * `grads`, times `scale`) — in ascending Gaussian order into `segment`:
 *   32-bit words [0] rows stored = min(needed, capacity), [1] rows needed, [2] N, [3] row_floats,
 *   [4 .. 4 + ceil(N/256)] first row of every block of 256 Gaussians, then (16-byte aligned) `capacity` rows of
 *   row_floats = riggs_grad_rows_row_floats(...) floats (index bits first, zero padded to a multiple of 4).
 * The caller all-gathers the segments of all ranks (equal riggs_grad_rows_segment_bytes) and calls
 * riggs_grad_rows_unpack: per Gaussian the rows are combined IN RANK ORDER — first occurrence overwrites, later ones are
 * added; rows in no segment are left as they are (zero on every rank) — without atomics, so every rank obtains the same
 * bits.  `grads` are HOST arrays of DEVICE pointers to (N, widths[k]) row-major float tensors (<= 8).  `status` (8 words;
 * [4] = THIS call's flag — [1]'s bits for this call alone, rewritten every call: the word a step's optimizers gate on; [0..3])
 * is STICKY — only ever raised by the kernel, cleared by whoever reads it: [0] = the largest number of rows a segment
 * needed, [1] != 0 when in some call a segment overflowed `capacity` or did not match (N, row_floats) (bit 0) or was marked
 * "frame invalid" by riggs_grad_rows_pack_gated (bit 1): in that call NOTHING
 * was unpacked (the gradients kept their local values) and the caller has to exchange that step densely — or, when it polls
 * only every k steps and the optimizers have already stepped on un-averaged gradients, re-synchronise the replicas; [2] = calls
 * since it was cleared, [3] = the call (1-based) that failed first.
 * `backward_workspace` is the workspace the last riggs_raster_backward of these N Gaussians used, on the same stream. */
int32_t riggs_grad_rows_row_floats(int32_t n_tensors, const int32_t* widths);
size_t riggs_grad_rows_segment_bytes(int32_t num_points, int32_t row_floats, int32_t capacity);
int riggs_grad_rows_pack(int32_t num_points, const void* backward_workspace, int32_t n_tensors, const float* const* grads,
                         const int32_t* widths, float scale, int32_t capacity, void* segment, riggs_stream stream);
int riggs_grad_rows_pack_gated(int32_t num_points, const void* backward_workspace, int32_t n_tensors, const float* const* grads,
                               const int32_t* widths, float scale, int32_t capacity, void* segment, const riggs_gate* gate,
                               riggs_stream stream);
/* backward_workspace (may be NULL): when given, the rows written are recorded in it as "rows that hold a gradient", which
 * keeps cfg.sparse_zero of the next riggs_raster_backward valid (rows other ranks touched are zeroed there when due). */
int riggs_grad_rows_unpack(int32_t num_points, int32_t world, int32_t capacity, const void* segments, int32_t n_tensors,
                           float* const* grads, const int32_t* widths, uint32_t* status, void* backward_workspace,
                           riggs_stream stream);
/* Test / measurement aid (multi-GPU readiness on one GPU): n_cus workgroups that each claim a whole compute unit's LDS — so they
 * sit on n_cus distinct CUs, as a collective library's channel kernels do beside a rank's frame — and spin until the host raises
 * *stop_flag (a DEVICE word, raised by a fill on another stream: pinned host memory is not coherent for a running kernel by default) or max_ms have passed (bounded).  *started (device u32, zeroed by the
 * caller) counts the workgroups that are resident.  Launch it on a stream of its own. */
int riggs_debug_pin_cus(int32_t n_cus, const int32_t* stop_flag, uint32_t max_ms, uint32_t* started, riggs_stream stream);

/* =====================================================================
 * Image loss: utils/loss_utils.py:17-18 (l1_loss), :33-77 (ssim, 11x11 Gaussian window,
 * sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over all elements), used at train_rig.py:508-509.
 * image / gt are (C, H, W) float32.  forward writes out3 = {l1 = mean |image - gt|, ssim = mean ssim_map,
 * (1 - lambda_dssim) l1 + lambda_dssim (1 - ssim)} (device; the third is the trainer's loss_img, train_rig.py:509) and
 * keeps three derivative maps + per-workgroup partial sums in `state` (riggs_l1_ssim_state_floats floats); backward
 * takes the upstream gradients of the three scalars as DEVICE scalars (NULL = 0) and writes dL/dimage (C, H, W).
 * ===================================================================== */
size_t riggs_l1_ssim_state_floats(int32_t C, int32_t H, int32_t W);
int riggs_l1_ssim_forward(int32_t C, int32_t H, int32_t W, const float* image, const float* gt, float lambda_dssim,
                          float* state, float* out3, riggs_stream stream);
int riggs_l1_ssim_backward(int32_t C, int32_t H, int32_t W, const float* image, const float* gt, const float* state,
                           float lambda_dssim, const float* g_l1, const float* g_ssim, const float* g_loss,
                           float* dL_dimage, riggs_stream stream);

/* =====================================================================
 * Optical-flow supervision of a stage-1 iteration (train_gui.py:1078-1121).
 *
 * Flow colours of gaussian_renderer.render_flow (gaussian_renderer/__init__.py:186-202), per Gaussian n:
 *   p_k = xyz[n] + d_xyz_k[n],  h_k = [p_k, 1] . full_proj_k,  u_k = h_k.xyz / h_k.w  (plain division, no + 1e-7),
 *   colour[n] = (u_2.x - u_1.x, u_2.y - u_1.y, motion_mask[n])
 * xyz is a constant (the reference detaches it).  d_xyz1 / d_xyz2 (N, 3) may be NULL (a residual of 0.0).  full_proj1 /
 * full_proj2 are DEVICE (4, 4) matrices in row-vector convention, the 16 floats the rasterizer reads as column-major
 * (pass the same pointer twice when there is no second camera).  motion_mask[n] = sigmoid(mask_logit[n * mask_logit_stride])
 * (the last column of the (N, fea_dim) feature: pointer to its first element, stride fea_dim), or 1 when mask_logit is NULL.
 * backward recomputes the projections (nothing is saved) and writes dL/dd_xyz1, dL/dd_xyz2 (N, 3) and dL/dmask_logit (N,
 * contiguous); each may be NULL.  A row whose incoming (dL/dcolour.x, dL/dcolour.y) is exactly zero gets exact zeros in both
 * residual gradients, whatever its h.w (the reference yields 0 * inf = NaN at h.w = 0), and dL/dmask_logit is exactly zero
 * where dL/dcolour.z is.  N = 0 is a no-op.
 *
 * Flow loss (train_gui.py:1101-1120), per pixel, image / gt (C, H, W), motion (3, H, W) (planes 0, 1 are read), alpha (H, W),
 * flow (H, W, 2) in RAFT pixels (8-byte aligned), masks (H, W, mask_channels >= 2) (channels 0, 1 are read):
 *   c = flow / (W, H) * 2;  live = alpha > 0.9 and (masks.0 > 0 or masks.1 > 0)
 *   w = live * clamp(cos(|fid1 - fid2| pi / 2), 0.2, 1) * cos(mean_c |image - gt| pi / 2)
 *   loss = mean over (H, W, 2) of |w c - w motion|
 * fid1 / fid2: DEVICE scalars fid1_dev / fid2_dev, or, where that pointer is NULL, the float passed by value.  forward writes
 * the loss (device scalar) and keeps w and the per-workgroup partial sums in `state` (riggs_flow_loss_state_floats floats);
 * the partials are added in a fixed order (bitwise repeatable).  backward takes the upstream gradient as a DEVICE scalar and
 * writes dL/dmotion (3, H, W), its third plane zero; a pixel with w = 0 gets exact zeros.
 * ===================================================================== */
int riggs_flow_colors_forward(int32_t N, const float* xyz, const float* d_xyz1, const float* d_xyz2, const float* full_proj1,
                              const float* full_proj2, const float* mask_logit, int64_t mask_logit_stride, float* colour,
                              riggs_stream stream);
int riggs_flow_colors_backward(int32_t N, const float* xyz, const float* d_xyz1, const float* d_xyz2, const float* full_proj1,
                               const float* full_proj2, const float* mask_logit, int64_t mask_logit_stride,
                               const float* dL_dcolour, float* dL_dd_xyz1, float* dL_dd_xyz2, float* dL_dmask_logit,
                               riggs_stream stream);
size_t riggs_flow_loss_state_floats(int32_t H, int32_t W);
int riggs_flow_loss_forward(int32_t C, int32_t H, int32_t W, int32_t mask_channels, const float* image, const float* gt,
                            const float* motion, const float* alpha, const float* flow, const float* masks,
                            const float* fid1_dev, const float* fid2_dev, float fid1, float fid2, float* state, float* loss,
                            riggs_stream stream);
int riggs_flow_loss_backward(int32_t H, int32_t W, const float* motion, const float* flow, const float* state,
                             const float* g_loss, float* dL_dmotion, riggs_stream stream);

/* =====================================================================
 * Skeleton projection loss: TrainRig.cal_skeleton_loss, train_rig.py:309-314, =
 * sampling_skeleton_points (:264-276) -> project_nodes_to_2d_elements (utils/other_utils.py:101-127) ->
 * pytorch3d.loss.chamfer_distance(x, y, norm=1) (third-party; restated from its published definition).
 * S line parameters t (the host evaluates the reference's int(max_len / (sum_len / 512)) and linspace) on each of the
 * J-1 bones of the posed joints d_nodes (J, 3); world_view_transform is the camera's (4, 4) matrix as the reference
 * stores it (row-vector convention, DEVICE pointer); fx, fy, cx, cy as other_utils.py:107-117 computes them; thinned is
 * the frame's (M, 2) silhouette-skeleton pixels as (row, col).  forward writes loss2 = {loss, weight * loss} (device;
 * `weight` is the trainer's robust per-frame weight of train_rig.py:465-467 as a DEVICE scalar, NULL = 1) and keeps the
 * nearest-neighbour keys in `state` (riggs_skeleton_projection_state_floats floats, 8-byte aligned); backward takes the
 * upstream gradients of the two scalars as DEVICE scalars (NULL = 0) and writes dL/d(d_nodes) (J, 3).  Deterministic
 * (the only atomics are 64-bit max and LDS integer adds).  pixel_count: optional DEVICE int32 (1 <= count <= M): the number
 * of valid rows of `thinned`, M then being the buffer's capacity — one captured graph serves frames of any pixel count.
 * ===================================================================== */
size_t riggs_skeleton_projection_state_floats(int32_t J, int32_t S, int32_t M);
int riggs_skeleton_projection_forward(int32_t J, int32_t S, int32_t M, const int32_t* parents, const float* d_nodes,
                                      const float* t, const float* world_view_transform, float fx, float fy, float cx,
                                      float cy, const float* thinned, const int32_t* pixel_count, const float* weight, float* state,
                                      float* loss2, riggs_stream stream);
int riggs_skeleton_projection_backward(int32_t J, int32_t S, int32_t M, const int32_t* parents, const float* d_nodes,
                                       const float* t, const float* world_view_transform, float fx, float fy, float cx,
                                       float cy, const float* thinned, const int32_t* pixel_count, const float* weight,
                                       float* state, const float* g_loss, const float* g_weighted, float* grad_nodes,
                                       riggs_stream stream);
/* The node projection term of stage 1 (train_gui.py:1133-1139): the point set is the J >= 1 rows of d_nodes themselves (the
 * control nodes: no bones, no sampling), projected by project_nodes_to_2d_elements and compared with `thinned` (M, 2) by the same
 * two-sided L1 chamfer distance (mean over the points of each side, summed).  Kernels of its own: the entry points above compute
 * what they always did.  Arguments as above; `state` holds riggs_node_projection_state_floats(J, M) floats, 8-byte aligned.
 * Deterministic. */
size_t riggs_node_projection_state_floats(int32_t J, int32_t M);
int riggs_node_projection_forward(int32_t J, int32_t M, const float* d_nodes, const float* world_view_transform, float fx, float fy,
                                  float cx, float cy, const float* thinned, const int32_t* pixel_count, const float* weight,
                                  float* state, float* loss2, riggs_stream stream);
int riggs_node_projection_backward(int32_t J, int32_t M, const float* d_nodes, const float* world_view_transform, float fx, float fy,
                                   float cx, float cy, const float* thinned, const int32_t* pixel_count, const float* weight,
                                   float* state, const float* g_loss, const float* g_weighted, float* grad_nodes,
                                   riggs_stream stream);

/* =====================================================================
 * Stage-1 control-node deformation, per-Gaussian part: ControlNodeWarp.cal_nn_weight
 * (utils/time_utils.py:934-964) + the blend of ControlNodeWarp.forward (:1138-1191) for skinning = False,
 * node_trans_bias = None, pred_opacity = pred_color = False.  pytorch3d.ops.knn_points (third-party) is restated as
 * "K smallest squared distances, ascending, ties to the lowest index".
 * x (N, 3); feature (N, feat_stride), its first `hyper` columns are the hyper coordinates (NULL and hyper = 0: xyz only);
 * motion_mask (N) or NULL (= 1); nodes (M, node_stride) = xyz then hyper coordinates; node_radius_log = _node_radius,
 * node_weight_logit = _node_weight (NULL: with_node_weight = False); node_trans / node_rot / node_scale / local_rot are the
 * node network's d_xyz (M, 3), d_rotation (M, 4), d_scaling (M, 3), local_rotation (M, 4; raw, (1,0,0,0) is added inside).
 * flags: 1 = local_frame, 2 = d_rot_as_res.  K <= 8, hyper <= 11, M (3 + hyper rounded up to 4) floats <= 128 KB.
 * forward writes d_xyz, d_rotation, d_scaling and cal_nn_weight's nn_idx (int32), nn_weight, nn_dist (N, K).
 * backward takes upstream gradients (each may be NULL = 0) and writes the gradients of feature (N, feat_stride; columns
 * beyond `hyper` zero), motion_mask, the node attributes, _node_radius, _node_weight and the nodes' hyper coordinates
 * (M, hyper); xyz of Gaussians and nodes are detached in the reference (:944, :947-949, :1152).  workspace:
 * riggs_cnode_backward_workspace_floats = 33 N K + max(1, ceil(N K / 4096)) M + M + 1 + 8 floats, 16-byte aligned; M <= 4096.
 * N = 0: every per-Gaussian pointer may be NULL (an empty tensor has no storage); the forward returns, the backward writes
 * zero node gradients.
 * ===================================================================== */
size_t riggs_cnode_backward_workspace_floats(int32_t N, int32_t M, int32_t K, int32_t hyper);
int riggs_cnode_forward(int32_t N, int32_t M, int32_t K, int32_t hyper, int32_t feat_stride, int32_t node_stride, int32_t flags,
                        const float* x, const float* feature, const float* motion_mask, const float* nodes,
                        const float* node_radius_log, const float* node_weight_logit, const float* node_trans,
                        const float* node_rot, const float* node_scale, const float* local_rot, float* d_xyz, float* d_rot,
                        float* d_scale, int32_t* nn_idx, float* nn_weight, float* nn_dist, riggs_stream stream);
int riggs_cnode_backward(int32_t N, int32_t M, int32_t K, int32_t hyper, int32_t feat_stride, int32_t node_stride, int32_t flags,
                         const float* x, const float* feature, const float* motion_mask, const float* nodes,
                         const float* node_radius_log, const float* node_weight_logit, const float* node_trans,
                         const float* node_rot, const float* node_scale, const float* local_rot, const int32_t* nn_idx,
                         const float* nn_dist, const float* g_xyz, const float* g_rot, const float* g_scale,
                         float* g_feature, float* g_motion_mask, float* g_node_trans, float* g_node_rot, float* g_node_scale,
                         float* g_local_rot, float* g_node_radius_log, float* g_node_weight_logit, float* g_nodes_hyper,
                         float* workspace, riggs_stream stream);
/* ---- Playback of a time track (inference only: no backward exists; ControlNodeWarp.deform_sequence).  Added symbols:
 * RIGGS_ABI_VERSION is unchanged.
 * riggs_cnode_sequence_forward: riggs_cnode_forward for T frames over ONE canonical cloud in one launch.  cal_nn_weight does
 * not depend on time, so a thread scans the nodes for its Gaussian once and keeps its K indices, normalised weights and the K
 * nodes' xyz in registers (the device code of riggs_cnode_forward: nn_idx and nn_dist equal its bit for bit); then it walks
 * the frames, gathers its K nodes' records of frame f from node_trans (T,M,3), node_rot (T,M,4), node_scale (T,M,3) and
 * local_rot (T,M,4; NULL without local_frame) and writes row (f, i) of d_xyz (T,N,3), d_rot (T,N,4), d_scale (T,N,3):
 * frame-major, a frame is contiguous.  nn_idx, nn_weight, nn_dist (N,K) are written once.  Limits and flags are those of
 * riggs_cnode_forward; T M <= 2^29; node_rot, local_rot and d_rot 16-byte aligned (they move as float4).  T = 0 or N = 0: no
 * launch, the per-Gaussian pointers may be NULL.
 * riggs_cnode_sequence_pass_frames: the frames the kernel takes per pass — 1: it has no passes, a frame's records are
 * gathered straight from the (T,M,.) tables, which stay in L2. */
int riggs_cnode_sequence_forward(int32_t N, int32_t M, int32_t T, int32_t K, int32_t hyper, int32_t feat_stride,
                                 int32_t node_stride, int32_t flags, const float* x, const float* feature,
                                 const float* motion_mask, const float* nodes, const float* node_radius_log,
                                 const float* node_weight_logit, const float* node_trans, const float* node_rot,
                                 const float* node_scale, const float* local_rot, float* d_xyz, float* d_rot, float* d_scale,
                                 int32_t* nn_idx, float* nn_weight, float* nn_dist, riggs_stream stream);
int32_t riggs_cnode_sequence_pass_frames(int32_t M, int32_t flags);

/* =====================================================================
 * Stage-1 node regularisers (csrc/node_reg.hip): ControlNodeWarp.arap_loss / elastic_loss / acc_loss
 * (utils/time_utils.py:1080-1120) over cal_connectivity_from_points / cal_arap_error (utils/deform_utils.py:51-103, 187-198).
 * Neighbour lists are padded (M, K) int32 with -1 for dropped edges; nothing is compacted.  M <= 8192, T <= 16, K <= 15.
 * Every backward is deterministic (no float atomics); losses are single device floats, upstream gradients device pointers.
 *
 * riggs_node_knn: for each of M points (D <= 16 coordinates, row stride `stride` floats) the Kq <= 16 smallest squared distances
 * to all M points, ascending, ties to the lowest index; column 0 dropped when drop_first; with radius2 > 0, columns
 * >= least_edge_num (after the drop) whose distance is not below radius2 become -1 / inf.  Columns beyond the point count are
 * -1 / inf.  Writes nn_idx, nn_dist (M, Kq - drop_first).
 * riggs_arap_*: seq (T, M, 3) node positions (t = 0 the source), nn_idx (M, K), rows (Ns) sample rows; forward writes the
 * rotations rot (Ns, T, 9; t = 0 unused) and loss = sum_{s, t >= 1, n} |tgt - R src|^2 over kept edges; backward holds rot
 * constant and writes g_seq (T, M, 3).  workspace: riggs_arap_workspace_floats floats.
 * riggs_elastic_*: nodes_t (M, T, 3), nn_idx (M, K), weight (M, K): loss = mean_m sum_k w var_T|edge| / (var + 1e-5) (unbiased
 * variance, the denominator held constant); backward writes g_nodes_t (M, T, 3) and g_weight (M, K).
 * riggs_acc_*: nodes_t (M, 3, 3): loss = mean_m |n0 + n2 - 2 n1| / (that + 1e-5); backward writes g_nodes_t (M, 3, 3).
 * ARAP / elastic: neighbour and sample-row indices outside [0, M) count as dropped edges (they are never dereferenced).
 * ===================================================================== */
int riggs_node_knn(int32_t M, int32_t D, int32_t stride, int32_t Kq, int32_t drop_first, int32_t least_edge_num, float radius2,
                   const float* points, int32_t* nn_idx, float* nn_dist, riggs_stream stream);
size_t riggs_arap_workspace_floats(int32_t M, int32_t T, int32_t K, int32_t Ns);
int riggs_arap_forward(int32_t M, int32_t T, int32_t K, int32_t Ns, const float* seq, const int32_t* nn_idx, const int32_t* rows,
                       float* rot, float* loss, float* workspace, riggs_stream stream);
int riggs_arap_backward(int32_t M, int32_t T, int32_t K, int32_t Ns, const float* seq, const int32_t* nn_idx, const int32_t* rows,
                        const float* rot, const float* g_loss, float* g_seq, float* workspace, riggs_stream stream);
size_t riggs_elastic_workspace_floats(int32_t M, int32_t T, int32_t K);
int riggs_elastic_forward(int32_t M, int32_t T, int32_t K, const float* nodes_t, const int32_t* nn_idx, const float* weight,
                          float* loss, float* workspace, riggs_stream stream);
int riggs_elastic_backward(int32_t M, int32_t T, int32_t K, const float* nodes_t, const int32_t* nn_idx, const float* weight,
                           const float* g_loss, float* g_nodes_t, float* g_weight, float* workspace, riggs_stream stream);
size_t riggs_acc_workspace_floats(int32_t M);
int riggs_acc_forward(int32_t M, const float* nodes_t, float* loss, float* workspace, riggs_stream stream);
int riggs_acc_backward(int32_t M, const float* nodes_t, const float* g_loss, float* g_nodes_t, riggs_stream stream);

/* =====================================================================
 * Stage-1 node network (csrc/node_mlp.hip): DeformNetwork (utils/time_utils.py:310-458) in fp32 on the matrix pipe.
 *   x_emb = PE_10(x) (63 columns); is_blender: t_emb = timenet(PE_6(t)) (13 -> 256 -> ReLU -> 30), else PE_10(t) (21);
 *   trunk: 8 Linear + ReLU of `width`, the embedded input concatenated in front of the output of layer 4;
 *   heads on the last activation: warp (3), scaling (3; max_d_scale > 0: tanh(.) * log(max_d_scale)), rotation (4),
 *   local_rotation (4, optional), opacity (1, optional): head_w / head_b in that order, NULL for an absent head.
 * Every weight is the fp32 master, row-major (out, in) as nn.Linear keeps it, and is read in place by every call: no copy is
 * kept, so nothing can go stale when an optimizer writes the masters between two calls.
 * width in {64, 128, 256}, depth 8, 1 <= R <= 65536 rows per call; anything else is rejected.  x (R, 3); t: R floats
 * (t_stride 1) or one float shared by every row (t_stride 0).  The inputs are not differentiated.
 * forward (one launch) writes the head outputs (contiguous (R, 3 / 3 / 4 / 4 / 1); a pointer per head present, NULL otherwise)
 * and `acts` (riggs_node_mlp_acts_floats floats: the embedded input, the time net's hidden row, the eight post-ReLU
 * activations; the last of them, the reference's `hidden` (R, width), starts at float riggs_node_mlp_hidden_offset).
 * backward (two launches) takes one cotangent per head (NULL: zero) and writes EVERY parameter gradient (overwriting) through
 * `grads`, shaped like the parameters; `workspace`: riggs_node_mlp_backward_workspace_floats floats.  Deterministic: each
 * (layer, 32 x 32 tile) of a weight gradient is one workgroup whose four waves walk the four quarters of the rows in ascending
 * order, added in wave order; no float atomics.
 * No host synchronisation, no allocation: capturable into a hipGraph.
 * ===================================================================== */
typedef struct riggs_node_mlp {
  int32_t width, depth, is_blender;
  float max_d_scale;                       /* <= 0: the scaling head is returned as it is */
  const float *tn_w0, *tn_b0, *tn_w1, *tn_b1; /* timenet.0 (256, 13), timenet.2 (30, 256); is_blender only */
  const float* w[8];                       /* linear.0 .. linear.7 */
  const float* b[8];
  const float* head_w[5];                  /* gaussian_warp, gaussian_scaling, gaussian_rotation, local_rotation, gaussian_opacity */
  const float* head_b[5];
} riggs_node_mlp;
typedef struct riggs_node_mlp_grads {
  float *tn_w0, *tn_b0, *tn_w1, *tn_b1;
  float* w[8];
  float* b[8];
  float* head_w[5];
  float* head_b[5];
} riggs_node_mlp_grads;
size_t riggs_node_mlp_acts_floats(int32_t R, int32_t width, int32_t depth);
size_t riggs_node_mlp_hidden_offset(int32_t R, int32_t width, int32_t depth);
size_t riggs_node_mlp_backward_workspace_floats(int32_t R, int32_t width, int32_t depth);
int riggs_node_mlp_forward(const riggs_node_mlp* net, int32_t R, const float* x, const float* t, int32_t t_stride, float* acts,
                           float* d_xyz, float* d_scaling, float* d_rotation, float* local_rotation, float* d_opacity,
                           riggs_stream stream);
int riggs_node_mlp_backward(const riggs_node_mlp* net, int32_t R, const float* acts, const float* g_xyz, const float* g_scaling,
                            const float* g_rotation, const float* g_local_rotation, const float* g_opacity, float* workspace,
                            const riggs_node_mlp_grads* grads, riggs_stream stream);

/* =====================================================================
 * simple_knn._C.distCUDA2 (scene/gaussian_model.py:20,170): mean squared distance to the 3
 * nearest neighbours.  points (P,3) -> out (P,).  workspace: riggs_knn_workspace_bytes(P).
 * ===================================================================== */
size_t riggs_knn_workspace_bytes(int32_t num_points);
int riggs_dist2_knn3(int32_t num_points, const float* points, float* out, void* workspace, riggs_stream stream);
/* the exact all-pairs search riggs_dist2_knn3 uses below 2048 points, callable at any size: the grid search's test oracle */
int riggs_dist2_knn3_bruteforce(int32_t num_points, const float* points, float* out, riggs_stream stream);

/* =====================================================================
 * Densification / pruning of the Gaussian cloud on the device (SURVEY.md §2 row 6 "next") — scene/gaussian_model.py:
 * densify_and_prune :500-514, densify_and_clone :475-498, densify_and_split :440-473, prune_points :373-392 and the optimizer
 * surgery around them (:338-417), called every densification_interval iterations at train_rig.py:359-365.
 *   riggs_densify_select   the three predicates of ONE densify_and_prune call as byte flags (3, N): [0] the old row survives
 *                          (not split, not pruned), [1] a clone of it is made and survives, [2] its split children survive
 *                          (grads = accum / denom with NaN -> 0; clone: |grad| >= thr and max scale <= dense_limit; split: grad
 *                          >= thr and max scale > dense_limit; prune: sigmoid(opacity) < min_opacity or, with world_limit >= 0,
 *                          max scale > world_limit — the children with their scale / child_div; the reference's screen-size
 *                          test never fires there: densification_postfix has zeroed max_radii2D by then)
 *   riggs_compact_indices  ascending indices of the set flags + their number (device int32), three launches, no atomics
 *   riggs_rows_gather      dst[t][m, :] = src[t][plan[m], :] for up to 32 tensors in ONE launch; plan[m] < 0 marks a NEW row made
 *                          from source ~plan[m]: tensors with zero_new[t] (the Adam moments) get zeros there
 *   riggs_split_children   the children's position R(q_parent) (z * scale_parent) + xyz_parent and log(scale_parent / child_div)
 *                          (z: unit normals, (n_children, 3); child j has parent parents[j % n_parents]: copy-major like .repeat(N, 1))
 * ===================================================================== */
int riggs_densify_select(int32_t num_points, int32_t scaling_columns, const float* xyz_gradient_accum, const float* denom,
                         const float* scaling, const float* opacity, float grad_threshold, float dense_limit, float min_opacity,
                         float world_limit, float child_div, uint8_t* flags, riggs_stream stream);
size_t riggs_compact_workspace_bytes(int32_t num_points);
int riggs_compact_indices(int32_t num_points, const uint8_t* flags, int32_t* out_indices, int32_t* count, void* workspace,
                          riggs_stream stream);
int riggs_rows_gather(int32_t n_out, const int32_t* plan, int32_t n_tensors, const float* const* src, float* const* dst,
                      const int32_t* row_floats, const uint8_t* zero_new, riggs_stream stream);
int riggs_split_children(int32_t n_children, int32_t n_parents, int32_t scaling_columns, const int32_t* parents,
                         const float* unit_normals, const float* xyz, const float* scaling, const float* rotation, float child_div,
                         float* new_xyz, float* new_scaling, riggs_stream stream);

/* =====================================================================
 * Dual-quaternion blending of rigid transforms — utils/dual_quaternion.py: QT2DQ :135-143, DQ2QT :146-165,
 * DQBlending :168-179 (what these two entry points compute), interpolate :182-187 and transformation_blending :190-197
 * (host compositions of them: riggs_amd/dual_quaternion.py).  The reference never calls the module on the skeleton path
 * (SURVEY.md §0.3); BASELINE.json's north_star names it, so it is here as an operator of its own.
 *   shared != 0: ONE set of K <= 1024 transforms for all rows — q (K, 4) raw quaternions (w, x, y, z), t (K, 3),
 *                weights (N, K): skinning.   shared == 0: every row has its own K <= 8 — q (N, K, 4), t (N, K, 3), weights (N, K).
 *   norm_over_nodes: QT2DQ normalises with torch.nn.functional.normalize(q), whose default axis is dim=1 — the quaternion
 *                axis of a 2-D q (0 here), the NODE axis of a 3-D q (1 here: every component is divided by its norm over the K
 *                nodes).  Both are the reference's results for the respective input rank.
 *   out_mode 0: out_rot (N, 9) row-major rotation matrix (rot_as_q=False), 1: out_rot (N, 4) through matrix_to_quaternion
 *                (rot_as_q=True; no sign standardisation), 2: out_rot (N, 16) = [R | t; 0 0 0 1] and out_t unused.
 * The dual part of a node is standardize_quaternion((0, t) * q) / 2 as in the reference (its sign does not follow q's).
 * Backward: cotangents in the layout of the outputs (g_t NULL = zeros; ignored with out_mode 2); dL_dq / dL_dt in the shape
 * of q / t, dL_dweights (N, K) or NULL; deterministic (no atomics).  workspace: riggs_dqb_backward_workspace_floats floats.
 * ===================================================================== */
int riggs_dqb_forward(int32_t num_rows, int32_t K, int32_t shared, int32_t norm_over_nodes, int32_t out_mode, const float* q,
                      const float* t, const float* weights, float* out_rot, float* out_t, riggs_stream stream);
size_t riggs_dqb_backward_workspace_floats(int32_t num_rows, int32_t K, int32_t shared);
int riggs_dqb_backward(int32_t num_rows, int32_t K, int32_t shared, int32_t norm_over_nodes, int32_t out_mode, const float* q,
                       const float* t, const float* weights, const float* g_rot, const float* g_t, float* dL_dq, float* dL_dt,
                       float* dL_dweights, float* workspace, riggs_stream stream);

/* =====================================================================
 * Kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 * `mask` has bit i set to time stage i; 0 disables (default: no events, no overhead).
 * riggs_prof_read synchronises on the recorded events and returns the sum / count since the
 * last riggs_prof_reset.  Stage ids: riggs_prof_name(i) for i in [0, riggs_prof_count()).
 * ===================================================================== */
/* debugging aid: per-wave statistics of the forward compositing kernel (8 u64 per wave, 4 waves per work item — a work
 * item is one pixel block of one tile = one workgroup, in launch order: {100 MHz ticks of the compositing loop, rounds,
 * survivors | hardware id << 32, steps, steps with a contribution, list length | tile << 32 | wide << 63, start tick, 0}),
 * followed (at word n_items * 32; n_items = riggs_raster_set_trace_items, default 8 per tile) by 4 u64 per chunk of the
 * compositing backward ({start, end, hardware id, workgroup << 32 | tile << 16 | chunk}); tools/fwd_trace.py, bwd_trace.py.
 * (How many tiles the forward may composite with 32 lanes per pixel and from which walk depth: riggs_set_option.)
 * NULL disables */
int riggs_raster_set_trace(void* dev_u64);
int riggs_raster_set_trace_items(uint64_t n_items);
/* =====================================================================
 * Per-Gaussian MLP heads on the matrix cores: WeightMLP / DeformMLP of
 * skeleton_utils/network_utils.py:6-112 as one fused launch per direction — 16-bit operands, fp32 accumulation
 * (v_mfma_f32_32x32x16_bf16 / _f16).  Every "bf16" buffer below holds the format the `fp16` argument selects, the same in
 * all five calls: 0 = bfloat16 (fp32's range, 8 significand bits), 1 = IEEE half (11 significand bits: parameter gradients
 * within 1-2 % of the fp32 arithmetic instead of 3-11 %, same rate; its range is the caller's business — see g_scale).
 * x_emb_bf16 (N rounded up to 128, in_pad) bf16, zero padded -> depth x [Linear(256) + ReLU], the embedding
 * re-concatenated IN FRONT of the hidden vector after layer `skip` (network_utils.py:58-61, 103-106) -> Linear(out_ch <= 32).
 * weights_bf16[l]: the 256 x K_l weights (K_0 = in_pad, K_{skip+1} = in_pad + 256 with the embedding columns first, else 256;
 * in_pad = in_ch rounded up to 64, padding columns zero) in the kernels' FRAGMENT-MAJOR order — [neuron tile T of 32][K-step s
 * of 16][lane 0..63][8 values], value j of a lane = W[32 T + (lane & 31)][16 s + 8 (lane >> 5) + j]: the 1 KB a wave loads per
 * (tile, step) is one contiguous run; w_out_bf16: the head alike, one tile of 32 outputs (>= out_ch zero) x 16 steps.
 * riggs_mlp_pack produces all of them from the fp32 masters; no caller needs to know the order.
 * acts_bf16 (depth, N, 256) receives the post-ReLU activations (operand of the weight gradients) and relu_masks
 * (depth, ceil(N / riggs_mlp_rows_per_workgroup()), 256) x 16 bytes their signs in the kernels' accumulator layout, for
 * riggs_mlp_backward (both NULL for inference).
 * n_rows_dev (riggs_mlp_forward / _backward / _wgrad; may be NULL): a device int32 — only rows < min(*n_rows_dev, N) exist; N
 * stays the row stride of acts_bf16 / dpre_bf16 and sizes the grid (the rest of the workgroups leave at once).  This is how the
 * row-sparse backward runs inside a hipGraph on the rows riggs_mlp_live_rows compacted, their number known to the device only.
 * Opt-in on the host side (riggs_amd.mlp): the reference computes these MLPs in fp32.
 * ===================================================================== */
/* Output epilogue of riggs_mlp_forward (host struct, may be NULL = the head's plain value), applied by the launch that holds the
 * value anyway instead of elementwise launches behind it:
 *   sigmoid:  out = sigmoid(head)  — WeightMLP (network_utils.py:107); the backward then multiplies the cotangent by
 *             out (1 - out) (riggs_mlp_live_rows / riggs_mlp_cotangent: sigmoid_out);
 *   res_base / res_mask / res_out:  res_out[n][c] = res_base[n][c] + out[n][c] * res_mask[n]  ((N, out_ch), (N) or NULL = 1,
 *             (N, out_ch)) — DeformMLP: the template offsets join the blended translation in front of the motion mask
 *             (skeleton_warp.py:152-161); the backward's counterpart is riggs_mlp_cotangent's g_rows / row_mask. */
struct riggs_mlp_epilogue {
  int32_t sigmoid;
  int32_t reserved;
  const float* res_base;
  const float* res_mask;
  float* res_out;
};
int riggs_mlp_forward(int32_t N, int32_t in_ch, int32_t out_ch, int32_t depth, int32_t skip,
                      const void* const* weights_bf16, const float* const* biases, const void* w_out_bf16,
                      const float* b_out, const void* x_emb_bf16, void* acts_bf16, void* relu_masks, float* out,
                      const int32_t* n_rows_dev, const struct riggs_mlp_epilogue* epilogue, int32_t fp16, riggs_stream stream);
/* Data-gradient pass of the same MLP: g_out (N, out_ch) = dL/d(output) -> dpre_bf16 (depth, N, 256) = dL/d(pre-activation)
 * of every hidden layer, the operand of the weight gradients  dW_l = dpre_l^T · input_l ,  db_l = sum_n dpre_l
 * (riggs_mlp_wgrad).  weights_t_bf16[l] (l >= 1): W_l[:, hidden part]^T (rows = the units of layer
 * l - 1), 256 x 256 values, fragment-major as above; w_out_t_bf16: W_out^T (rows = hidden units, 32 padded outputs as
 * inputs), fragment-major.  No gradient w.r.t. x_emb (detached in the reference).
 * g_scale (device scalar, may be NULL = 1): g_out is multiplied by it on load, so dpre and db_partial come out scaled by it —
 * with fp16 the caller passes a power of two that lifts max|g_out| to ~2^10 (loss-scaled gradients: a per-pixel-averaged
 * loss leaves |g_out| ~ 1e-7, below half precision's normal range) and divides the parameter gradients by it. */
int riggs_mlp_backward(int32_t N, int32_t out_ch, int32_t depth, int32_t skip, const void* const* weights_t_bf16,
                       const void* w_out_t_bf16, const float* g_out, const float* g_scale, const void* relu_masks,
                       void* dpre_bf16, float* db_partial, const int32_t* n_rows_dev, int32_t fp16, riggs_stream stream);
/* Row-sparse backward, step 1: the rows of g_out (N, out_ch) that hold a non-zero — the Gaussians the render gave a gradient;
 * the WeightMLP has no other cotangent: its regulariser is dead code at train_rig.py:433-444, and the skinning backward writes
 * exact zeros for the rest — in ascending order: live_idx (N) their indices, live_count (device int32) their number M,
 * x_live_bf16 ((N rounded up to 128), in_pad) the gathered rows of x_emb_bf16 (zero-filled up to the next multiple of 128
 * behind row M), g_live (N, out_ch) the gathered rows of g_out.  Two launches, no atomics (deterministic).  A zero row
 * contributes zero to every data gradient, bias sum and weight product, so riggs_mlp_forward (activations of the live rows
 * only: the first forward then stores none), riggs_mlp_backward and riggs_mlp_wgrad on (x_live, g_live, n_rows_dev =
 * live_count) return the parameter gradients of the dense pass.  workspace: riggs_mlp_live_rows_workspace_bytes(N), 8-byte
 * aligned.
 * sigmoid_out (N, out_ch; may be NULL): the head's output went through riggs_mlp_epilogue.sigmoid — the cotangent of the head is
 * g_out * s (1 - s), which is what is tested for a non-zero and gathered into g_live (no sigmoid_backward launch in front).
 * scale (device float; may be NULL): receives the fp16 gradient scale of riggs_mlp_cotangent over that cotangent — per-block
 * maxima from the first launch, reduced by the second: no launch and no atomic of its own. */
size_t riggs_mlp_live_rows_workspace_bytes(int32_t N);
int riggs_mlp_live_rows(int32_t N, int32_t out_ch, int32_t in_ch, const float* g_out, const float* sigmoid_out, const void* x_emb_bf16,
                        void* workspace, int32_t* live_idx, int32_t* live_count, void* x_live_bf16, float* g_live, float* scale,
                        riggs_stream stream);
/* The cotangent the data-gradient pass reads, for an (N, out_ch) head, and the g_scale of the fp16 format taken from it — two
 * launches, no host synchronisation:
 *   g_eff = (g + g_rows * row_mask[row]) * [s (1 - s)] + l2_coef[0] * l2_out
 *   scale[0] = 2^floor(log2(1024 / max|g_eff|))   (max|g_eff| clamped at 1e-30)
 * g, g_rows (N, out_ch): at least one; row_mask (N; NULL = 1; needs g_rows): the motion mask that multiplied the head's output on
 * its way into res_out (riggs_mlp_epilogue); sigmoid_out (N, out_ch; NULL = no factor): the head's sigmoid-ed output;
 * l2_out / l2_coef (both or neither): an L2 regulariser on the MLP's OUTPUT — the template offsets' term of the stage-2
 * objective, train_rig.py:446-454: lambda * mean(template_offsets^2) over all Gaussians (x1e3 on the template frame); l2_out is
 * that output, l2_coef a device scalar = 2 lambda / (N out_ch), refreshed by the host between replays; mean_sq[0] (may be NULL)
 * then receives mean(l2_out^2), the value the reference logs.
 * g_eff may be NULL exactly when the cotangent is g itself (g given; g_rows, sigmoid_out and l2_out NULL): g is read for its
 * maximum and nothing but scale is written.  Anything else with g_eff == NULL is refused.
 * zero_word: a device u32 that is ZERO on entry (the caller clears it once) and zero again behind the call; partials512: 512
 * floats of scratch.  g, l2_out and g_eff 16-byte aligned; N * out_ch < 2^31 (a flat tensor of n floats: N = n, out_ch = 1). */
int riggs_mlp_cotangent(int32_t N, int32_t out_ch, const float* g, const float* g_rows, const float* row_mask,
                        const float* sigmoid_out, const float* l2_out, const float* l2_coef, float* g_eff, float* scale,
                        uint32_t* zero_word, float* partials512, float* mean_sq, riggs_stream stream);
/* db_partial: (ceil(N / riggs_mlp_rows_per_workgroup()), depth, 256) fp32 — per-workgroup column sums of dpre; the bias
 * gradients are their sum over the first axis.  May be NULL when riggs_mlp_wgrad follows (it sums the columns itself). */
int32_t riggs_mlp_rows_per_workgroup(void);
/* The parameter gradients of one MLP from what the two passes left in memory, in three launches: every product
 *   dW_l = dpre_l^T · input_l   (input_0 = x_emb, input_l = acts_{l-1}; layer skip + 1: [x_emb | acts_skip]),
 *   dW_out = (g_out · g_scale)^T · acts_{depth-1},   db_l = sum_n dpre_l,   db_out = sum_n g_out · g_scale
 * streamed once by one workgroup per CU (split over the Gaussians, fp32 accumulators, LDS-direct loads — mlp_wgrad.hip), the
 * split partials summed, divided by g_scale (NULL = 1) and written to the fp32 tensors torch.autograd hands back:
 * grad_weights[l] (256, K_true) row-major with K_true = in_true / in_true + 256 (layer skip + 1) / 256, in_true = in_ch + tail_ch,
 * grad_biases[l] (256), grad_w_out (out_ch, 256), grad_b_out (out_ch).  x_emb_bf16 / acts_bf16 / dpre_bf16: the buffers of
 * riggs_mlp_forward / riggs_mlp_backward, same format.  workspace: riggs_mlp_wgrad_workspace_bytes bytes, 256-byte aligned,
 * contents irrelevant (depends on N, the shape and the device's CU count).
 * tail_ch / tail: an MLP whose input ends in tail_ch values that are THE SAME FOR EVERY ROW (DeformMLP: the pose vector,
 * skeleton_warp.py:152 `pose = local_rot.detach().reshape(-1)[None].expand(N, -1)`): the masters' weights of the two layers that
 * read the input have in_ch + tail_ch input columns, the packed operands and x_emb_bf16 only the first in_ch (riggs_mlp_pack with
 * the same tail_ch); the gradient of the tail's columns is (bias gradient) x tail — written by the launch that sums the
 * partials.  tail: tail_ch floats on the device.  tail_ch = 0 with tail = NULL: the plain MLP. */
size_t riggs_mlp_wgrad_workspace_bytes(int32_t N, int32_t in_ch, int32_t depth, int32_t skip);
int riggs_mlp_wgrad(int32_t N, int32_t in_ch, int32_t tail_ch, const float* tail, int32_t out_ch, int32_t depth, int32_t skip,
                    const void* x_emb_bf16, const void* acts_bf16, const void* dpre_bf16, const float* g_out, const float* g_scale,
                    void* workspace, size_t workspace_bytes, float* const* grad_weights, float* const* grad_biases,
                    float* grad_w_out, float* grad_b_out, const int32_t* n_rows_dev, int32_t fp16, riggs_stream stream);
/* fp32 master weights ((256, K_true) row-major per layer, (out_ch, 256) for the head) -> every bf16 operand the two kernels
 * read (layouts above), in one launch.  tail_ch > 0 (riggs_mlp_wgrad): K_true = in_ch + tail_ch (+ 256 in layer skip + 1), and
 * the tail's columns are left out of the packed operands. */
int riggs_mlp_pack(int32_t in_ch, int32_t tail_ch, int32_t out_ch, int32_t depth, int32_t skip, const float* const* weights,
                   const float* w_out, void* const* weights_bf16, void* const* weights_t_bf16, void* w_out_bf16,
                   void* w_out_t_bf16, int32_t fp16, riggs_stream stream);
/* ... and what they contribute: bias_eff (2, 256) = [b_first + W_first[:, in_ch : in_ch + tail_ch] tail,
 * b_skip + W_skip[:, in_ch : in_ch + tail_ch] tail] in fp32 — the biases riggs_mlp_forward takes for layer 0 and layer skip + 1
 * (network_utils.py:46-51: h = cat([x_emb, t_emb]) enters both).  One launch per forward: the tail changes with every frame. */
int riggs_mlp_tail_bias(int32_t in_ch, int32_t tail_ch, const float* w_first, const float* b_first, const float* w_skip,
                        const float* b_skip, const float* tail, float* bias_eff, riggs_stream stream);
/* The kernels' input operand from positions: row n = [x_n, sin(2^k x_n), cos(2^k x_n) for k < multires, tail (n_tail floats,
 * the same for every row: DeformMLP's pose), 0 ...] as bf16, (N rounded up to 128) x (width rounded up to 64)
 * (utils/time_utils.py:208-256 get_embedder + the concatenation of network_utils.py:40-46). */
int riggs_mlp_embed(int32_t N, int32_t multires, int32_t n_tail, const float* x, const float* tail, void* out_bf16,
                    int32_t fp16, riggs_stream stream);
/* self-test of the MFMA fragment layouts mlp.hip assumes: writes D = A B for A = [I_16; 0] and an asymmetric B */
int riggs_mlp_layout_probe(float* out32x32, riggs_stream stream);

/* Farthest-point sampling (csrc/fps.hip; utils/time_utils.py:461-482, bit for bit: nearest starts at 1e10, squared distance
 * fl(fl(dx dx + dy dy) + dz dz) without fused multiply-add, update on dist < nearest, next point = the maximum of nearest with
 * the LOWEST index on ties, the start index first in the output).  xyz: N rows of 3 fp32, row_stride floats apart (>= 3);
 * start: one device int64, read by the first launch (clamped to [0, N)): nothing synchronises; workspace:
 * riggs_fps_workspace_bytes(N) bytes, 256-byte aligned, contents irrelevant (nearest and the per-workgroup partials);
 * out_indices: npoint device int64.  One plain launch per picked point over riggs_fps_blocks(N) workgroups (sized from N: one
 * workgroup up to 1024 points); no grid barrier, no cooperative launch.  npoint may exceed N (the sweep then repeats indices as
 * the reference does). */
int32_t riggs_fps_blocks(int32_t N);
size_t riggs_fps_workspace_bytes(int32_t N);
int riggs_fps_sample(int32_t N, int32_t npoint, const float* xyz, int64_t row_stride, const int64_t* start, void* workspace,
                     int64_t* out_indices, riggs_stream stream);
/* The same sweep over rows of D fp32, 1 <= D <= 64 (the stage-1 node sampling over 16-sample trajectories: D = 48), row_stride
 * floats apart (>= D).  Squared distance: the sequential fp32 sum ((t_0^2 + t_1^2) + t_2^2) + ... over ascending columns with
 * t_k = fl(p_k - c_k), every product and sum rounded: at D = 3 the indices of riggs_fps_sample.  The rows are transposed once per
 * call into a (D, N) image inside the workspace (riggs_fps_rows_workspace_bytes(N, D) bytes, 256-byte aligned: 4 N D bytes for the
 * image on top of nearest and the partials), then one plain launch per picked point.  start, out_indices, npoint as above. */
size_t riggs_fps_rows_workspace_bytes(int32_t N, int32_t D);
int riggs_fps_sample_rows(int32_t N, int32_t D, int32_t npoint, const float* rows, int64_t row_stride, const int64_t* start,
                          void* workspace, int64_t* out_indices, riggs_stream stream);

/* =====================================================================
 * Evaluation report: L1, PSNR, SSIM and MS-SSIM of B frames (C, H, W) against their ground truth, as train_utils.py:56-243 and
 * render_rig.py:111-218 report them.  SSIM is piq.ssim(x, y, data_range=1.): mean pool by f = max(1, round(min(H, W) / 256))
 * (half to even), then one level with a VALID 11 x 11 Gaussian window (sigma 1.5), mean of ssim_map over the outputs and the
 * channels.  MS-SSIM is pytorch_msssim.ms_ssim(X, Y, data_range=1.): five such levels with a 2 x 2 mean pool (h % 2, w % 2 zeros
 * in front, counted in the divisor) between them, prod_l relu(v_l) ^ wt_l per channel (v = the cs mean of levels 0..3 and the
 * ssim mean of level 4; wt = 0.0448, 0.2856, 0.3001, 0.2363, 0.1333), mean over channels; needs min(H, W) > 160.  Both are
 * restated from the packages' published algorithms.  PSNR = 20 log10(1 / sqrt(mean (x - y)^2)) per frame (inf for identical
 * images), L1 = mean |x - y|.  clamp != 0 clamps both inputs to [0, 1] first (the reference's torch.clamp before its metrics).
 * out: (B, 4) = {l1, psnr, ssim, ms_ssim} per frame (ms_ssim = NaN unless want_ms_ssim).  levels_or_null: (B, 6, C, 2) =
 * {ssim mean, cs mean} of the five MS-SSIM levels and of the piq level (NaN for a level the call did not compute).
 * workspace: riggs_image_metrics_workspace_floats(B, C, H, W) floats, 8-byte aligned.  Every sum is formed in a fixed order in
 * float64: a frame's row does not depend on B or on the other frames.  All launches go on `stream`; nothing synchronises.
 * Layout of the workspace after the call (a promise: tests/test_gpu_ssim_window_f64.py reads it).  First the per-workgroup partial
 * sums as float64, level by level (levels 0..4 = the MS-SSIM pyramid, planned whenever min(H, W) > 160; level 5 = the pooled piq
 * level, absent when f = 1, where level 0 serves): [plane = b * C + c][workgroup = by * tx + bx][4] = {sum ssim_map, sum cs_map,
 * sum |x - y|, sum (x - y)^2 (the last two on level 0 only, else 0)}, a workgroup being 32 columns x 64 rows of the level's
 * (h - 10) x (w - 10) outputs.  Then, as float32, the images of levels 1..5 in that order: x's B * C planes, then y's, each (h, w)
 * with h_l = ceil(h_{l-1} / 2) (likewise w) for l = 1..4 and H / f, W / f for l = 5.  Parts of a level the call did not compute
 * (want_ms_ssim = 0) are left as they were.
 * Rejected before any HIP call (non-zero status, riggs_last_error): B < 1 or C < 1, a NULL x / y / out / workspace, a workspace
 * that is too small, want_ms_ssim with min(H, W) <= 160, an SSIM level smaller than 11 on a side after pooling.
 * ===================================================================== */
size_t riggs_image_metrics_workspace_floats(int32_t B, int32_t C, int32_t H, int32_t W);
int riggs_image_metrics(int32_t B, int32_t C, int32_t H, int32_t W, const float* x, const float* y, int32_t clamp,
                        int32_t want_ms_ssim, float* out, float* levels_or_null, float* workspace, size_t workspace_floats,
                        riggs_stream stream);

/* =====================================================================
 * The editor's display frame (riggs_amd/viewer.py): interactive_GUI.py::test_step :497-664 with its overlay builders :97-247,
 * render_rig.py::project_nodes_to_2d_withnodes :40-94 and utils/other_utils.py::depth2normal :78-97.  Inference only; every
 * launch goes on `stream`, nothing synchronises.  Added symbols: RIGGS_ABI_VERSION is unchanged.
 *
 * A PRIMITIVE is RIGGS_VIEWER_PRIM_WORDS = 12 32-bit words: [0] kind (segment / disc / axis-aligned square), [1..4] the integer
 * end points x0 y0 x1 y1 (a disc's centre twice; a square's left_top and right_bottom), [5] the DOUBLED extent of the colour
 * shape and [6] of the alpha shape (a segment's thickness t, a disc's 2 r; unused by squares), [7..9] rgb as float bits, [10]
 * valid, [11] reserved (0).  A table lists primitives in paint order; the last writer wins.
 *
 * COVERAGE.  OpenCV's own scan conversion is not restated; the rule is geometric.  The pixel at integer (x, y) is inside
 *   a disc of radius r at the integer centre c     iff  dx^2 + dy^2 <= r^2;
 *   a square                                        iff  x0 <= x <= x1 and y0 <= y <= y1 (the reference's left_top .. right_bottom);
 *   a segment of thickness t                        iff  its squared distance to the CLOSED segment is <= (t / 2)^2 (round caps);
 *   a zero-length segment is a disc of radius t / 2.
 * With e2 the doubled extent this is evaluated in integers as 4 d^2 <= e2^2 against an end point (or the centre) and
 * 4 cross^2 <= e2^2 |b - a|^2 against the body.  Coordinates are clamped to +-RIGGS_VIEWER_COORD_MAX = 8192 (which only moves
 * end points that lie that far off screen; the window is at most that large) and e2 <= RIGGS_VIEWER_EXT2_MAX = 4096, so every
 * product stays below 2^61: exact in int64.  A primitive with a non-finite coordinate or w <= 0 (z <= 0 under the render_rig
 * rule) is marked invalid and never drawn — a deviation: OpenCV would draw garbage there.
 * ===================================================================== */
#define RIGGS_VIEWER_PRIM_WORDS 12
#define RIGGS_VIEWER_COORD_MAX 8192
#define RIGGS_VIEWER_EXT2_MAX 4096
#define RIGGS_VIEWER_MAX_TABLES 8
#define RIGGS_VIEWER_RANGE_WORKSPACE_FLOATS 512
enum { RIGGS_VIEWER_SEGMENT = 0, RIGGS_VIEWER_DISC = 1, RIGGS_VIEWER_SQUARE = 2 };
enum { RIGGS_VIEWER_RULE_EDITOR = 0, RIGGS_VIEWER_RULE_RENDER_RIG = 1 };
enum { RIGGS_VIEWER_LAYOUT_SKELETON = 0, RIGGS_VIEWER_LAYOUT_SQUARES = 1, RIGGS_VIEWER_LAYOUT_POLYLINES = 2 };
enum { RIGGS_VIEWER_MODE_IMAGE = 0, RIGGS_VIEWER_MODE_DEPTH = 1, RIGGS_VIEWER_MODE_ALPHA = 2, RIGGS_VIEWER_MODE_NORMAL = 3 };
enum { RIGGS_VIEWER_BLEND_ALPHA = 0, RIGGS_VIEWER_BLEND_MASK = 1 };

/* min and max of n floats into out_min_max[0], [1]: two fixed-order stages, no atomics; exact, a NaN wins as in torch.min / max.
 * workspace: RIGGS_VIEWER_RANGE_WORKSPACE_FLOATS floats. */
int riggs_viewer_depth_range(int64_t n, const float* depth, float* workspace, float* out_min_max, riggs_stream stream);

/* depth2normal: depth (h, w) -> out (3, h, w), unit normals; focal as the reference's default w / 2 / tan(pi / 6) or given. */
int riggs_viewer_depth2normal(int32_t h, int32_t w, const float* depth, float focal, float* out, riggs_stream stream);

/* Points -> primitives, one launch.  rule EDITOR: uv = (p_hom @ matrix)[:2] / w with matrix = full_proj_transform, then
 * (uv + 1) / 2 * [scale_x, scale_y] where the reference passes scale_x = image_height and scale_y = image_width (x scaled by the
 * HEIGHT: kept); RENDER_RIG: matrix = world_view_transform, fx x / z + cx + 0.5 and fy y / z + cy + 0.5.  Both truncate toward
 * zero.  Layouts (the count is riggs_viewer_project_count):
 *   SKELETON   points (n, 3), parents (n): n - 1 segments (joint i -> parents[i], i >= 1; colour rgb[0..2], thickness
 *              segment_ext2) and n discs (colours[i] or rgb[3..5]; doubled radii disc_color_ext2 / disc_alpha_ext2); the segments
 *              come first unless discs_first.  uv, if given, receives the n un-truncated coordinates (n, 2).
 *   SQUARES    points (n, 3): trunc(uv - square_radius) .. trunc(uv + square_radius), colours[i] or rgb[0..2]; uv as above.
 *   POLYLINES  points (ring_capacity, n, 3), a ring of samples whose oldest is slot ring_head: for each of the n tracks the
 *              samples - 1 segments between consecutive samples, track after track; colours[track] or rgb[0..2].
 * table may be NULL when only uv is wanted. */
typedef struct riggs_viewer_projection {
  int32_t layout, rule, n, samples, ring_head, ring_capacity, discs_first;
  int32_t segment_ext2, disc_color_ext2, disc_alpha_ext2, square_radius, reserved;
  const float* points;
  const int32_t* parents;
  const float* matrix; /* (4, 4) row-major, on the device */
  const float* colors; /* or NULL */
  float scale_x, scale_y, fx, fy, cx, cy;
  float rgb[6];
  int32_t* table;
  float* uv;
} riggs_viewer_projection;
int64_t riggs_viewer_project_count(const riggs_viewer_projection* p);
int riggs_viewer_project(const riggs_viewer_projection* p, riggs_stream stream);

/* The display frame, one launch (a 16 x 16 tile per workgroup).  Base colour by mode — IMAGE: source (3, h, w); DEPTH: source
 * (1, h, w) as (d - min) / (max - min + 1e-20) with range = {min, max} on the device; ALPHA: source (1, h, w) replicated; NORMAL:
 * (depth2normal(source) + 1) / 2, evaluated at the source pixels the taps read — then F.interpolate(mode="bilinear",
 * align_corners=False) to (height, width) (scale_h = h / height and scale_w = w / width, in float) and a clamp to [0, 1].  The
 * tables are then painted one after another: per table a colour layer (rgb where the pixel is in a primitive's colour shape) and
 * an alpha layer (1 where it is in its alpha shape), then BLEND_ALPHA: out = base (1 - a) + rgb a, or BLEND_MASK:
 * out = base (sum(rgb) == 0) + rgb.  out: (height, width, 3) float32. */
typedef struct riggs_viewer_frame {
  int32_t mode, src_height, src_width, height, width, num_tables;
  float focal, scale_h, scale_w;
  int32_t reserved;
  const float* source;
  const float* range;
  const int32_t* tables[RIGGS_VIEWER_MAX_TABLES];
  int32_t counts[RIGGS_VIEWER_MAX_TABLES];
  int32_t rules[RIGGS_VIEWER_MAX_TABLES];
  float* out;
} riggs_viewer_frame;
int riggs_viewer_compose(const riggs_viewer_frame* f, riggs_stream stream);

/* =====================================================================
 * 2-D skeleton thinning of silhouette masks (csrc/thin.hip; riggs_amd/thinning.py): what process_data/cal_2d_skeleton.py makes
 * offline with skimage.morphology.thin and scene/dataset_readers.py reads back as viewpoint_cam.thinned.  Guo and Hall's
 * two-subiteration parallel thinning, restated from the published algorithm (the conditions are spelled out in csrc/thin.hip);
 * it reproduces the published 7 x 7 example of skimage's documentation, agreement with an installed skimage beyond that is not
 * verified.  Integer only; images are bytes, set = non-zero on input and 1 on output.  Added symbols: RIGGS_ABI_VERSION is
 * unchanged.
 *
 * Sub-iteration number n (from 0) applies table (first_subiter + n) % 2; after every second one an image stops if the pair
 * deleted nothing.  max_subiters < 0: until converged; otherwise exactly at most that many sub-iterations run.
 * PATH LDS: one workgroup per image keeps the bit plane in LDS, one launch for the batch, nothing synchronises.  PATH GLOBAL
 * (images whose plane does not fit): one launch per sub-iteration over planes in `workspace`
 * (riggs_thin_workspace_bytes(B, H, W, path) bytes, 256-byte aligned; 0 for the LDS path), and every check_every iterations the
 * host reads back the per-image deletion counters: this path synchronises `stream` and cannot be captured.  PATH AUTO takes
 * riggs_thin_path(H, W) (-1 for sizes outside 1 .. 32768).
 * ===================================================================== */
enum { RIGGS_THIN_PATH_AUTO = -1, RIGGS_THIN_PATH_LDS = 0, RIGGS_THIN_PATH_GLOBAL = 1 };
int32_t riggs_thin_path(int32_t H, int32_t W);
size_t riggs_thin_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t path);
int riggs_thin(int32_t B, int32_t H, int32_t W, const uint8_t* mask_u8, uint8_t* out_u8, int32_t first_subiter,
               int32_t max_subiters, int32_t path, int32_t check_every, void* workspace, riggs_stream stream);
/* The set (non-zero) pixels of B images (H, W) of bytes as float32 rows (row, col), each coordinate
 * (float)((double)v / resolution), in row-major ascending order (np.where's), one workgroup per image: points (B, capacity, 2),
 * counts (B) int32 = min(number of set pixels, capacity).  Rows at and beyond counts[b] are not written. */
int riggs_thin_elements(int32_t B, int32_t H, int32_t W, const uint8_t* img_u8, double resolution, int32_t capacity, float* points,
                        int32_t* counts, riggs_stream stream);

/* =====================================================================
 * Multiresolution hash-grid encoding (csrc/hashgrid.hip; riggs_amd/hash_network.py): the encoding of the reference's
 * HashDeformNetwork (utils/time_utils.py:517-571, 712-767), which it takes from tinycudann.Encoding ("Grid" / "Hash" / "Linear").
 * Restated from the published algorithm (Mueller et al., Instant Neural Graphics Primitives, 2022; tests/hashgrid_ref.py is the
 * NumPy restatement); tinycudann does not build for this platform, so agreement with its binary is NOT verified: checkpoint
 * exchange rests on the layout below and on the published algorithm.  Added symbols: RIGGS_ABI_VERSION is unchanged.
 *
 * D = n_input_dims in {3, 4}, L = n_levels in 1 .. 16, F = n_features_per_level = 2, log2_hashmap_size in 3 .. 24, linear
 * interpolation.  All integer arithmetic is uint32 with wrap-around.  Per level l:
 *   scale[l] = (float)(base_resolution * pow(per_level_scale, l) - 1)       (in double, rounded once)
 *   resolution[l] = ceil(scale[l]) + 1
 *   size[l] = min(round_up_8(resolution[l]^D), 2^log2_hashmap_size)          (the power exact, in 64 bits)
 *   hashed[l] = resolution[l]^D > size[l]   (0: a dense level);   offset[l] = size[0] + .. + size[l-1], offset[L] = the total
 * The table is (offset[L], F) fp32: level-major, entry-major, feature-minor.
 * Per row and level: pos_d = fmaf(scale, x_d, 0.5f), cell_d = (uint32)(int32)floorf(pos_d), frac_d = pos_d - floorf(pos_d); over
 * the 2^D corners c = cell + bit the weight is prod_d (bit_d ? frac_d : 1 - frac_d) and the entry is
 *   dense:  (sum_d c_d * resolution^d) % size        hashed:  (xor_d c_d * prime_d) % size,  primes {1, 2654435761, 805459861, 3674653429}
 * so every index is in range for any finite coordinate, also outside [0, 1] (taken as it comes, no clamp; |pos| < 2^31).
 * out (R, L F), column l F + f.  mask: L F floats or NULL; it multiplies the output in the forward and the cotangent in the
 * backward; a level whose two mask values are 0 is not gathered (its columns are 0) and not scattered.
 * backward ADDS w * mask * g_out[row][l F + f] into g_table (same layout as the table; the caller zeroes it) with float atomic
 * adds: the sum's order is the arrival order, so the table gradient can differ in its last bits from run to run.  The
 * coordinates are not differentiated.  x, table, out, g_out, g_table are device pointers, 8-byte aligned; 0 <= R < 2^31 / (L F).
 * Neither call allocates, reads back or synchronises.  riggs_hashgrid_levels_fill is host arithmetic only (no HIP call).
 * ===================================================================== */
#define RIGGS_HASHGRID_MAX_LEVELS 16
/* The per-level table is RIGGS_HASHGRID_TABLE_WORDS 32-bit words in HOST memory: [0] n_input_dims, [1] n_levels,
 * [2] n_features_per_level, [3] log2_hashmap_size, [4] the entries of the whole table (offset[L]), [5..7] 0, then
 * RIGGS_HASHGRID_LEVEL_WORDS words per level l at RIGGS_HASHGRID_HEADER_WORDS + 5 l: the bits of the float scale[l],
 * resolution[l], size[l], offset[l], hashed[l]. */
#define RIGGS_HASHGRID_HEADER_WORDS 8
#define RIGGS_HASHGRID_LEVEL_WORDS 5
#define RIGGS_HASHGRID_TABLE_WORDS 88
int riggs_hashgrid_levels_fill(int32_t n_input_dims, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size,
                               double base_resolution, double per_level_scale, uint32_t* levels /* host, TABLE_WORDS words */);
int riggs_hashgrid_forward(const uint32_t* levels /* host */, int32_t R, const float* x /*(R,D)*/, const float* table,
                           const float* mask /* or NULL */, float* out /*(R,L F)*/, riggs_stream stream);
int riggs_hashgrid_backward(const uint32_t* levels /* host */, int32_t R, const float* x /*(R,D)*/, const float* mask /* or NULL */,
                            const float* g_out /*(R,L F)*/, float* g_table, riggs_stream stream);

/* =====================================================================
 * A semantic label per control node (csrc/semantic.hip; riggs_amd/skeleton_init.py: node_semantic_labels), the input of the
 * skeleton extraction's symmetry pass.  Replaces, for all F training frames in one launch, what the trainer does camera by camera:
 *   TrainRig.init_skeleton_info / set_semantic_label   train_rig.py:129-131, 177-190, 215-216
 *   torch.median(nodes_semantic_label, dim=0).values.int()   train_rig.py:227
 * d_nodes (F, M, 3): the nodes at every frame; cameras: a DEVICE table of F records, record f the camera of frame f.
 * Per (f, m): (row, col) = (fy y / z + cy, fx x / z + cx) of the node in camera space, the projection of
 * riggs_node_projection_forward in the same fp32 steps (project_nodes_to_2d_elements, utils/other_utils.py:101-127); both
 * truncated toward zero; row >= H -> H - 1 and col >= W -> W - 1, THEN whatever is < 0 -> 0; labels[f][m] = map[row][col].
 * A record whose map is NULL (a camera without semantic_seg) gives 0 for its whole row f.  A projection that is not finite
 * (z = 0, a NaN node) is undefined in the reference; here it reads pixel (0, 0).
 * Outputs: labels (F, M) fp32, the reference's nodes_semantic_label; median (M,) int32, per node the LOWER median of its F
 * labels — the element of rank (F - 1) / 2, torch.median's rule — taken over the fp32 values and converted back, as the
 * reference does (exact for |label| <= 2^24).
 * 1 <= F <= RIGGS_SEMANTIC_MAX_FRAMES, 1 <= M <= RIGGS_SEMANTIC_MAX_NODES, else an error and no launch.  One launch of
 * ceil(M / T) workgroups of 256 threads with 4 F T <= 65536 bytes of LDS, T = riggs_node_semantic_tile(F) nodes per workgroup
 * (0 for an F out of range).  Does not allocate, read back or synchronise: legal inside a stream capture.  The maps (and the
 * table) must stay alive until the launch has run.  Added symbols: RIGGS_ABI_VERSION is unchanged.
 * ===================================================================== */
#define RIGGS_SEMANTIC_MAX_FRAMES 1024
#define RIGGS_SEMANTIC_MAX_NODES 65536
/* A camera record is RIGGS_SEMANTIC_CAMERA_WORDS 32-bit words (8-byte aligned): [0 .. 15] the floats of world_view_transform,
 * (4, 4) row-major as the reference stores it (row-vector convention); [16 .. 19] the floats fx, fy, cx, cy; [20], [21] int32
 * image_height H and image_width W, the shape of the map (1 <= H, W < 2^24; a record with H < 1 or W < 1 is read as one without
 * a map); [22 .. 23] the 64-bit device pointer to the (H, W) int32 map, or 0. */
#define RIGGS_SEMANTIC_CAMERA_WORDS 24
int32_t riggs_node_semantic_tile(int32_t F);
int riggs_node_semantic_labels(int32_t F, int32_t M, const float* d_nodes, const void* cameras /* device: F records */,
                               float* labels, int32_t* median, riggs_stream stream);

/* =====================================================================
 * Inverse kinematics on the rig's chain (csrc/ik.hip; riggs_amd/pose_edit.py: solve_ik): turn the joints so that up to
 * RIGGS_IK_MAX_HANDLES handle joints reach their targets.  Damped least squares (Wampler 1986) with the clamped target step of
 * Buss & Kim (2005), restated from the published method (the reference's editor turns one joint at a time and has no IK);
 * tests/ik_ref.py is the NumPy restatement.  Added symbols: RIGGS_ABI_VERSION is unchanged.
 *
 * B problems on one skeleton: joints (J,3), parents (J) as riggs_fk_forward takes them (parents[i] < i; a value outside [0, i)
 * is clamped into it), 1 <= J <= 256, 1 <= E <= RIGGS_IK_MAX_HANDLES.  Per problem b: local_rot_in (B,J,4) un-normalised wxyz,
 * global_trans_in (B,3), handles (B,E) joint indices, targets (B,E,3), weights (B,E) or NULL (all 1): a weight <= 0 (or NaN)
 * switches its handle off, and so does a handle index outside [0, J), whose residual is NaN.  locked (J) bytes or NULL: a joint
 * with a non-zero byte keeps its quaternion, bit for bit, as does every joint on no live handle's path root .. handle.
 * `iterations` >= 0 steps of: forward kinematics; per live handle d = target - posed, shortened to max_step, r = sqrt(w) d; the
 * Jacobian blocks -sqrt(w) [posed_handle - pivot_a]x of the unlocked joints a on the handle's path (pivot_a: the posed parent,
 * the root's own position), with solve_translation a further block sqrt(w) I; (J J^T + damping^2 I) y = r by Cholesky;
 * omega_a = J_a^T y turned into the parent's frame, theta = |.|, and q_a <- (cos theta/2, sin(theta/2) axis) (x) q_a where
 * theta > 0; global_trans += sum sqrt(w) y with solve_translation.  Then one more forward kinematics:
 * local_rot_out (B,J,4), global_trans_out (B,3), d_nodes (B,J,3) the posed joints, residual (B,E) = |target - posed handle|.
 * The outputs may alias the inputs of the same shape.
 * damping > 0 and max_step >= 0 are host values; bit 0 (bit 1) of `relative` multiplies damping (max_step) by the device float
 * *extent (read by the kernel: nothing is read back), which is only needed then.
 * One workgroup per problem, all iterations in ONE launch on `stream` (J <= 64: one wave; else 256 threads); no float atomics:
 * the same inputs give the same bits, and a problem's result does not depend on the rest of the batch.  Does not allocate, read
 * back or synchronise: legal inside a stream capture.
 * ===================================================================== */
#define RIGGS_IK_MAX_HANDLES 8
int riggs_ik_solve(int32_t B, int32_t J, int32_t E, const float* joints, const int32_t* parents, const float* local_rot_in,
                   const float* global_trans_in, const int32_t* handles, const float* targets, const float* weights,
                   const uint8_t* locked, int32_t iterations, float damping, float max_step, const float* extent, int32_t relative,
                   int32_t solve_translation, float* local_rot_out, float* global_trans_out, float* d_nodes, float* residual,
                   riggs_stream stream);

/* =====================================================================
 * Whole-skeleton pose fitting (csrc/fit.hip; riggs_amd/pose_edit.py: fit_pose): EVERY joint may have a target position, which the
 * dual form of riggs_ik_solve (a 3E x 3E factorisation on one wave) cannot carry.  Levenberg-Marquardt (Levenberg 1944, Marquardt
 * 1963) with Buss & Kim's clamped target step, the damped normal equations solved matrix-free by Jacobi-preconditioned conjugate
 * gradients (Hestenes & Stiefel 1952); restated from the published methods, tests/fit_ref.py is the NumPy restatement.  Added
 * symbol: RIGGS_ABI_VERSION is unchanged.
 *
 * joints, parents, B, J, local_rot_in, global_trans_in, locked, damping, max_step, relative and the outputs are riggs_ik_solve's.
 * targets (B,J,3) and weights (B,J) or NULL (all 1): a weight <= 0 (or NaN) means that the joint has no target; its target is
 * never read (a NaN there changes nothing).  *extent (device float, > 0) is ALWAYS required: the translation unknown is
 * tau' = tau / extent, so that all unknowns carry length units.  cg_steps >= 1.
 * `iterations` >= 0 steps of (s_h = sqrt(w_h), 0 without target; piv_a = posed_vp(a), the root's own position; a subtree
 * includes its root; positions relative to the posed root, pc = posed - posed_0, which changes neither operator):
 *   1  forward kinematics; r_h = s_h (target_h - posed_h, shortened to max_step)
 *   2  J p:    W_j = W_vp(j) + omega_j (a locked joint's omega is 0), C_j = C_vp(j) + omega_j x piv_j,
 *              u_h = s_h ((W_h x pc_h - C_h) + extent tau')
 *      J^T u:  F_a = sum_subtree s_h u_h, M_a = sum_subtree pc_h x (s_h u_h), g_a = M_a - piv_a x F_a (locked: 0),
 *              g_tau' = extent F_0;  A = J^T J + damping^2 I;  a parent adds its children in descending index
 *   3  Minv_a = 1 / (2/3 d_a + damping^2), d_a = sum_subtree s_h^2 |pc_h - piv_a|^2 = max((S2 - 2 piv_a . S1) + |piv_a|^2 S0, 0)
 *      from the subtree moments S0, S1, S2 of s^2, s^2 pc, s^2 |pc|^2 ABOUT THE POSED ROOT (every term is then within one rig
 *      extent of the others, wherever global_trans is);  Minv_tau' = 1 / (extent^2 S0_0 + damping^2)
 *   4  cg_steps steps of preconditioned conjugate gradients from x = 0 on A x = J^T r.  Before a step it ends unless
 *      r.z > 1e-10 * (r.z at the start), and unless p.Ap > 0: the same decision in every thread.  A dot product is
 *      (a0 b0 + a1 b1) + a2 b2 per joint, a balanced binary tree over each 64 joints, the (up to four) sums in order, tau' last.
 *   5  riggs_ik_solve's step 5 with omega_a = x_a; global_trans += extent x_tau' with solve_translation
 * then one more forward kinematics: d_nodes (B,J,3) and residual (B,J) = |target - posed| where the joint has a target, else 0.
 * A locked joint keeps its quaternion bit for bit, as does a joint whose subtree holds no target.
 * One workgroup per problem, all iterations in ONE launch on `stream` (J <= 64: one wave; else 256 threads); no float atomics:
 * the same inputs give the same bits, and a problem's result does not depend on the rest of the batch.  Does not allocate, read
 * back or synchronise: legal inside a stream capture.
 * ===================================================================== */
int riggs_fit_pose(int32_t B, int32_t J, const float* joints, const int32_t* parents, const float* local_rot_in,
                   const float* global_trans_in, const float* targets, const float* weights, const uint8_t* locked,
                   int32_t iterations, int32_t cg_steps, float damping, float max_step, const float* extent, int32_t relative,
                   int32_t solve_translation, float* local_rot_out, float* global_trans_out, float* d_nodes, float* residual,
                   riggs_stream stream);

/* =====================================================================
 * Bone-direction fitting (csrc/bones.hip; riggs_amd/pose_edit.py: fit_bones, retarget): every bone h >= 1 (joint h and its parent)
 * may have a target DIRECTION, which does not depend on the proportions of the skeleton it was taken from: a motion-capture clip,
 * another rig's track, a rest skeleton extracted anew.  riggs_fit_pose's method on the unit bone vectors: Levenberg-Marquardt with
 * the clamped step, the damped normal equations solved matrix-free by Jacobi-preconditioned conjugate gradients; restated from the
 * published methods, tests/bones_ref.py is the NumPy restatement.  Added symbol: RIGGS_ABI_VERSION is unchanged.
 *
 * joints, parents, B, J (1 .. 256), local_rot_in, global_trans_in, locked and the outputs are riggs_fit_pose's.  directions (B,J,3):
 * a vector along the target of bone h in row h, of any length; row 0 is never read.  weights (B,J) or NULL (all 1).  Per problem,
 * once: L_h = |x_h - x_vp(h)|; row h is read only if weights[h] > 0 and L_h > 0; t_h = v_h / |v_h|; the target is live iff also
 * |v_h| > 0 (a NaN fails every comparison: off); s_h = sqrt(w_h) where live, else 0; S0_a = sum_subtree s_h^2 (a subtree includes
 * its root), Minv_a = 1 / (2/3 S0_a + damping^2).  damping > 0 and max_step >= 0 are absolute and dimensionless; cg_steps >= 1.
 * `iterations` >= 0 steps of:
 *   1  forward kinematics; beta_h = posed_h - posed_vp(h), d_h = beta_h / |beta_h| (live h, else 0);
 *      r_h = s_h (t_h - d_h, shortened to max_step)
 *   2  J p:    W_j = W_vp(j) + omega_j (a locked joint's omega is 0), u_h = s_h (W_h x d_h): the rig is rigid, a bone only turns
 *      J^T u:  g_a = sum_subtree d_h x (s_h u_h) (locked: 0);  A = J^T J + damping^2 I;  a parent adds its children in
 *              descending index
 *   3  cg_steps steps of preconditioned conjugate gradients from x = 0 on A x = J^T r, with riggs_fit_pose's two stopping rules
 *      (r.z > 1e-10 * (r.z at the start); p.Ap > 0) and its dot product: (a0 b0 + a1 b1) + a2 b2 per joint, a balanced binary
 *      tree over each 64 joints, the (up to four) sums in order
 *   4  riggs_ik_solve's step 5 with omega_a = x_a
 * then one more forward kinematics: d_nodes (B,J,3) and residual (B,J) = |t_h - d_h| where the target is live (the chord of two
 * unit vectors, in [0, 2]), else 0.  global_trans_out is global_trans_in: no translation is solved for.
 * A locked joint keeps its quaternion bit for bit, as does a joint whose subtree holds no live target.  The twist about a bone is
 * not observed; it stays where it was up to rounding.
 * One workgroup per problem, all iterations in ONE launch on `stream` (J <= 64: one wave; else 256 threads); no float atomics:
 * the same inputs give the same bits, and a problem's result does not depend on the rest of the batch.  Does not allocate, read
 * back or synchronise: legal inside a stream capture.
 * ===================================================================== */
int riggs_fit_bones(int32_t B, int32_t J, const float* joints, const int32_t* parents, const float* local_rot_in,
                    const float* global_trans_in, const float* directions, const float* weights, const uint8_t* locked,
                    int32_t iterations, int32_t cg_steps, float damping, float max_step, float* local_rot_out,
                    float* global_trans_out, float* d_nodes, float* residual, riggs_stream stream);

/* =====================================================================
 * Pose fitting to lines and points (csrc/rays.hip; riggs_amd/pose_edit.py: fit_rays, fit_keypoints): every joint may be held to up
 * to RIGGS_RAYS_MAX LINES (the ray through a camera centre and a 2-D keypoint; the editor's cursor) and to one POINT (a pin:
 * riggs_fit_pose's target).  riggs_fit_pose's method: Levenberg-Marquardt with the clamped step, the damped normal equations solved
 * matrix-free by Jacobi-preconditioned conjugate gradients.  The vector from a point to a line has the constant Jacobian
 * -(I - d d^T) with respect to the point, so riggs_fit_pose's weight s_h^2 becomes a symmetric 3 x 3 metric N_h per joint that does
 * not depend on the pose; two or more cameras triangulate and fit in one solve, with one camera the depth is held by the damping
 * alone.  Restated from the published methods, tests/rays_ref.py is the NumPy restatement.  Added symbol: RIGGS_ABI_VERSION is
 * unchanged.
 *
 * joints, parents, B, J (1 .. 256), local_rot_in, global_trans_in, locked, damping, max_step, *extent (always required), relative,
 * solve_translation, cg_steps and the outputs are riggs_fit_pose's.  0 <= K <= RIGGS_RAYS_MAX rays per joint: origins (B,J,K,3),
 * directions (B,J,K,3) of any length, ray_weights (B,J,K); all three NULL iff K == 0.  pins (B,J,3) and pin_weights (B,J): both
 * NULL = no pins (K == 0 needs them).  Per problem and joint h, once: ray k is live iff ray_weights > 0 and 0 < |direction| < inf
 * (a NaN fails every comparison: off), d = direction / |direction|; the pin is live iff pin_weights > 0 (wp_h, else 0).  Nothing
 * of a constraint that is not live is read beyond what decides that (the weight, then the direction): a NaN there changes nothing.
 *   N_h = wp_h I + sum_k w_hk (I - d_hk d_hk^T) (k ascending; 6 floats),  n_h = ((N_xx + N_yy) + N_zz) / 3
 * `iterations` >= 0 steps of riggs_fit_pose's iteration with
 *   1  per live ray e_k = v - (d . v) d, v = o_k - posed_h (from the joint to the nearest point of the line); the pin:
 *      e = pin_h - posed_h; each shortened to max_step on its own; f_h = sum_k w_hk e_k + wp_h e (k ascending, the pin last);
 *      the right-hand side is J^T f (riggs_fit_pose's up-sweep with f_h in place of s_h r_h)
 *   3  the moments S0, S1, S2 of n_h, n_h pc, n_h |pc|^2 in place of s_h^2 ...; Minv_tau' = 1 / (extent^2 S0_0 + damping^2)
 *   4  J p: u_h = (W_h x pc_h - C_h) + extent tau' (no weight);  J^T: F, M over the subtrees of N_h u_h and pc_h x (N_h u_h), with
 *      (N u)_x = (N_xx u_x + N_xy u_y) + N_xz u_z and so on;  A = J^T N J + damping^2 I
 * then one more forward kinematics: d_nodes (B,J,3) and residual (B,J) = the largest |e| (not shortened) over the joint's live
 * constraints, in world units; 0 where it has none.  A locked joint keeps its quaternion bit for bit, as does a joint whose
 * subtree holds no live constraint.  A line extends behind its origin; what is minimised is the distance to the line (the
 * reprojection error times depth / focal length), not the pixel error.
 * One workgroup per problem, all iterations in ONE launch on `stream` (J <= 64: one wave; else 256 threads); no float atomics:
 * the same inputs give the same bits, and a problem's result does not depend on the rest of the batch.  Does not allocate, read
 * back or synchronise: legal inside a stream capture.
 * ===================================================================== */
#define RIGGS_RAYS_MAX 8
int riggs_fit_rays(int32_t B, int32_t J, int32_t K, const float* joints, const int32_t* parents, const float* local_rot_in,
                   const float* global_trans_in, const float* origins, const float* directions, const float* ray_weights,
                   const float* pins, const float* pin_weights, const uint8_t* locked, int32_t iterations, int32_t cg_steps,
                   float damping, float max_step, const float* extent, int32_t relative, int32_t solve_translation,
                   float* local_rot_out, float* global_trans_out, float* d_nodes, float* residual, riggs_stream stream);

/* =====================================================================
 * Filters along the time axis of a pose track (csrc/track.hip; riggs_amd/track.py: smooth_track, one_euro_track, OneEuroTrack).
 * Inference only.  B tracks of T frames and J (1 .. RIGGS_TRACK_MAX_JOINTS) joints: rot_in (B,T,J,4) quaternions of any length
 * (q, -q and s q with s > 0 are one pose), 16-byte aligned; trans_in (B,T,3) or NULL = the translation is not filtered (then
 * trans_out and trans_weights are NULL too); weights (B,T,J) and trans_weights (B,T) confidences, NULL = all 1.  A rotation sample
 * is VALID iff its weight > 0 (a NaN fails the comparison) and 0 < |q|^2 < inf in float32 (not zero, NaN or infinite); a
 * translation sample iff its weight > 0 and its three components are finite.  Every other sample is a GAP: beyond what decides
 * that, nothing of it enters any output (the one exception is named below).  q^ = q / |q| with |q|^2 = ((w w + x x) + y y) + z z.
 * Outputs are unit quaternions.  One launch each on `stream`; no float atomics: the same inputs give the same bits, and a track's
 * result does not depend on the rest of the batch.  Neither allocates, reads back or synchronises: legal inside a stream capture.
 * Restated from the published methods; tests/track_ref.py is the NumPy restatement.  Added symbols: RIGGS_ABI_VERSION is unchanged.
 *
 * riggs_track_smooth: a confidence-weighted Gaussian window on SO(3).  taps (radius + 1) device floats g[d], g[0] first (the caller
 * evaluates exp(-d^2 / (2 sigma^2)); the kernel evaluates no exp); 0 <= radius <= RIGGS_TRACK_MAX_RADIUS.  The window of frame t is
 * s = t - radius .. t + radius in that order, clipped to [0, T), or with `wrap` taken modulo T (2 radius + 1 <= T is required).
 *   support[t,j] = sum_s w,  w = g[|s - t|] c[s,j]   over the window's valid samples (0 where there is none)
 *   M = sum_s (w q^_a) q^_b   (10 entries, a <= b)   the chordal L2 mean of the rotations is the unit eigenvector of M's largest
 *   eigenvalue (Markley, Cheng, Crassidis & Oshman 2007); M does not see a sample's sign.  Four cyclic Jacobi sweeps over the
 *   pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) in registers, no data-dependent exit; per pair theta = (a_qq - a_pp) / (2 a_pq),
 *   t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) (0 where a_pq = 0), c = 1 / sqrt(t^2 + 1), s = t c.  The column of the largest
 *   diagonal entry (the first on equality), normalised.  Sign: dot(out, q^_t) >= 0 where sample (t, j) is valid, else the first
 *   non-zero component is positive.
 *   trans_out[t] = (sum_s w p_s) / (sum_s w) with w = g[|s - t|] c[s] over the valid translation samples of the same window.
 * Without support (support = 0) rot_out is the input sample normalised where 0 < |q|^2 < inf - the one place a gap's quaternion is
 * read - else (1, 0, 0, 0), and trans_out the input row.  radius = 0 returns the normalised input.  One thread per (b, t, j),
 * adjacent threads on adjacent joints; joint 0's thread filters the frame's translation.
 *
 * riggs_track_one_euro: the one-euro filter (Casiez, Roussel & Vogel 2012), causal, one lane per (b, j) over the T frames and one
 * per track for the translation.  State, read and written in place (a call continues where the last one stopped: T frames in one
 * call and in two calls are the same code, and the same bits): state_rot (B,J,4) q^, state_omega (B,J), state_gap (B,J) frames
 * since the last valid sample, < 0 = none yet; state_trans (B,3), state_velocity (B,3), state_trans_gap (B) (NULL iff trans_in is).
 * A fresh state is state_gap = state_trans_gap = -1 and anything finite elsewhere.  alpha(f, dt) = 1 / (1 + 1 / ((2 pi f) dt)).
 * Per frame, a valid sample x = q^:  the first one sets q^ = x, omega^ = 0;  otherwise dt = (gap + 1) / rate, x = -x where
 * dot(x, q^) < 0, th = acos(min(|dot|, 1)), omega = 2 th / dt, a_d = alpha(d_cutoff, dt), omega^ = a_d omega + (1 - a_d) omega^,
 * a = alpha(min_cutoff + beta omega^, dt), q^ = slerp(q^, x, a) in riggs_pose_slerp's steps from its dot product on (the sin
 * weights, the linear ones where sin(th) <= 1e-6, the result normalised); gap = 0.  A gap frame keeps the state and raises gap.
 * rot_out[t] = q^, or (1, 0, 0, 0) before any sample.  The translation likewise on vectors: v = (p - p^) / dt,
 * v^ = a_d v + (1 - a_d) v^ per component, a = alpha(trans_min_cutoff + trans_beta |v^|, dt), p^ = a p + (1 - a) p^;
 * trans_out[t] = p^, or 0 before any sample.  rate, min_cutoff, d_cutoff, trans_min_cutoff > 0, beta, trans_beta >= 0, all finite.
 * ===================================================================== */
#define RIGGS_TRACK_MAX_RADIUS 64
#define RIGGS_TRACK_MAX_JOINTS 256
int riggs_track_smooth(int32_t B, int32_t T, int32_t J, int32_t radius, int32_t wrap, const float* rot_in, const float* trans_in,
                       const float* weights, const float* trans_weights, const float* taps, float* rot_out, float* trans_out,
                       float* support, riggs_stream stream);
int riggs_track_one_euro(int32_t B, int32_t T, int32_t J, const float* rot_in, const float* trans_in, const float* weights,
                         const float* trans_weights, float rate, float min_cutoff, float beta, float d_cutoff,
                         float trans_min_cutoff, float trans_beta, float* state_rot, float* state_omega, int32_t* state_gap,
                         float* state_trans, float* state_velocity, int32_t* state_trans_gap, float* rot_out, float* trans_out,
                         riggs_stream stream);

/* =====================================================================
 * ARAP handle editing of control nodes (csrc/arap.hip; riggs_amd/arap.py: ARAPDeformer, LapDeform): the drag of the reference's
 * utils/arap_deform.py, "these M nodes go there" -> positions and rotations of all N nodes.  Inference only.
 * B drags of ONE handle set over one graph.  verts (N,3) rest positions p0; nn_idx (N,K) neighbour lists, an entry outside [0,N)
 * is a dropped edge; weight (N,K) edge weights w, 0 on a dropped edge.  A = I - W is the reference's L_opt (A[i][nn[i][k]] = -w_ik).
 * op (N, op_ld) row-major, 16-byte aligned, op_ld a multiple of 4 with N <= op_ld <= 1024: the operator G whose rows of the
 * non-handle nodes are the rows of pinv(A_u), A_u = A's non-handle columns, and whose handle rows and columns >= N are zero.
 * handle_idx (M) distinct nodes; handle_pos (B,M,3) their targets; init_verts (B,N,3) or NULL.
 *   x_init = p0 with the handles on their targets.  Every solve is in displacement form, x = x_init + G (b - A x_init): a
 *   direction the handles do not determine (a dropped singular value of A_u) keeps its rest position, and a handle stays on its
 *   target bit for bit.  Where A_u has full rank this is the reference's lstsq_with_handles(A, b).
 *   The initial solve (skipped when init_verts is given: x = init_verts as it is) has b = A p0, so b - A x_init = A (p0 - x_init).
 *   Each of `iterations` (the reference runs 3) rounds, with P_ik = p0_i - p0_j, P'_ik = x_i - x_j over the kept edges j = nn[i][k]:
 *     S_i = sum_k w_ik P_ik P'_ik^T (float64);  R_i = the proper rotation that maximises tr(R S_i) (Horn's quaternion form,
 *     csrc/horn_rotation.h: the reference's W U^T with the Kabsch flip), or I where for at least one coordinate axis that
 *     coordinate of every edge is bit-equal at rest and now (arap_deform.py:133-134; a dropped edge counts as equal), or S = 0;
 *     b_i = 1/2 sum_k w_ik (R_i + R_j) P_ik;  x = x_init + G (b - A x_init).
 *   pos_out (B,N,3) = x; quat_out (B,N,4) or NULL = the R of the last round as (w,x,y,z) by matrix_to_quaternion's component rule
 *   (the best-conditioned candidate, no sign fix), (1,0,0,0) for iterations = 0.
 * One workgroup per drag, all rounds in ONE launch on `stream`; the 64 partial sums of a row of G meet in a fixed tree and there
 * are no float atomics: the same inputs give the same bits, and a drag's result does not depend on the rest of the batch.  Does not
 * allocate, read back or synchronise: legal inside a stream capture.  Added symbol: RIGGS_ABI_VERSION is unchanged.
 * ===================================================================== */
#define RIGGS_ARAP_EDIT_MAX_NODES 1024
#define RIGGS_ARAP_EDIT_MAX_K 16
int riggs_arap_edit(int32_t B, int32_t N, int32_t K, int32_t M, const float* verts, const int32_t* nn_idx, const float* weight,
                    const float* op, int32_t op_ld, const int32_t* handle_idx, const float* handle_pos, const float* init_verts,
                    int32_t iterations, float* pos_out, float* quat_out, riggs_stream stream);

int riggs_prof_count(void);
const char* riggs_prof_name(int32_t id);
int riggs_prof_enable(uint32_t mask);
int riggs_prof_reset(void);
int riggs_prof_read(int32_t id, float* total_ms, int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* RIGGS_HIP_H */
