/*
 * dpc_render.h -- C ABI of libdpc_render.so: the differentiable point-cloud projection of
 * NiteshBharadwaj/pytorch-unsup-pc as hand-written HIP kernels for MI355X (gfx950).
 *
 * The reference has no native code and no FFI: its hot path is Python calling ATen
 * (SURVEY.md section 2b).  The entry points below are therefore what a binding for that path would bind --
 * one call per reference function, plus the fused forward/backward that replaces the whole of
 * pointcloud_project_fast and its autograd graph.  Each entry cites the reference code it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - plain C, no C++/torch types; all pointers are DEVICE pointers unless named host_*;
 *   - every buffer is allocated by the caller; the library never allocates device memory and never
 *     synchronises the stream (so calls can be captured into a hipGraph);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - return value: DPC_OK (0) or a negative DPC_ERR_* code; dpc_strerror() names it;
 *   - B == 0 (no clouds: an empty shard) is valid everywhere: nothing is launched, array pointers may be NULL, and
 *     dpc_project_loss_fwd writes loss = 0;
 *   - re-entrant, no global state; arithmetic type fp32 (the ray-march transmittance product runs in fp64
 *     registers); tensors are dense row-major with the shapes stated per argument;
 *   - optional inputs (t, f, s) and optional outputs are NULL when absent;
 *   - grids, silhouettes and the workspace are read and written with 8- and 16-byte accesses: their base pointers must be
 *     16-byte aligned (anything hipMalloc returns is); the big grids a launch writes and does not read again (the W/H-
 *     filtered grid, its gradient) are stored write-through, which needs nothing from the caller.
 *
 * Grid: D x H x W voxels (D = vox_size_z or vox_size, H = W = vox_size), voxel (z,y,x) of cloud b at
 * [((b*D + z)*H + y)*W + x].  Point clouds are [B,N,3] xyz, quaternions [B,4] (w,x,y,z) unnormalised.
 */
#ifndef DPC_RENDER_H
#define DPC_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPC_ABI_VERSION 15
#define DPC_MAX_TAPS 63 /* longest 1-D smoothing kernel accepted (pc_gauss_kernel_size) */
/* Size limits, checked by every entry point (DPC_ERR_SHAPE): grid sides <= 1024 (10-bit cell indices in a point record),
 * B <= 65535, and N <= DPC_MAX_POINTS points per cloud: a voxel's splat weights are summed in 64-bit fixed point with 44
 * fractional bits, so 2^20 - 1 points of weight 1 in ONE voxel is the most that cannot wrap. */
#define DPC_MAX_POINTS 1048575
/* Most points per cloud of a dpc_emd_fwd pair: the auction keeps a pair in the 160 KiB of LDS of one CU at 76 bytes per
 * point (both clouds in fp64, prices, bids, owners), 152 KiB at this size. */
#define DPC_EMD_MAX_POINTS 2048
/* Most points per cloud of dpc_fps: a cloud is held on chip by one workgroup of 1024 threads, 16 points per thread. */
#define DPC_FPS_MAX_POINTS 16384
/* Longest side of a grid of the dpc_voxel* entry points: a 128^3 bit grid is 256 KiB, four LDS slabs of dpc_voxelise,
 * and a flat voxel index stays far inside an int. */
#define DPC_VOXEL_MAX_SIDE 128
/* dpc_voxel_edt: the value of every voxel of a grid without a seed (INT32_MAX; the largest real value is 3 * 127^2), and
 * the most thresholds of one dpc_voxel_edt_stats call. */
#define DPC_VOXEL_EDT_NONE 2147483647
#define DPC_VOXEL_EDT_MAX_THRESHOLDS 8
/* The fills of dpc_voxelise_meshes, and the size from which a vertex coordinate counts as not finite there (below it no
 * product of the separating-axis tests can overflow). */
#define DPC_MESH_FILL_NONE 0
#define DPC_MESH_FILL_CARVE 1
#define DPC_MESH_FILL_PARITY 2
#define DPC_MESH_VOXEL_MAX_COORD 18446744073709551616.0 /* 2^64 */
/* dpc_point_mesh_distance: the points of a workgroup (one lane each), the faces it stages in LDS per round, and the least
 * number of such tiles in a chunk of faces when a row's face range is split over workgroups. */
#define DPC_PM_BLOCK 256
#define DPC_PM_FACE_TILE 128
#define DPC_PM_CHUNK_TILES 8
/* dpc_mesh_winding: the fractional bits of a face's quantised term, and so of the int64 sums (the unit is 2^-40). */
#define DPC_WINDING_FRAC_BITS 40
/* dpc_ray_mesh_intersect: the LDS of a workgroup, DPC_PM_FACE_TILE staged faces of nine doubles padded to five double2. */
#define DPC_RAY_LDS_BYTES 10240
/* dpc_knn_batched / dpc_pca_normals: the most neighbours per query, and the references a workgroup stages in LDS per
 * round.  A workgroup holds DPC_KNN_BLOCK(k) queries, one lane each: 256 for k <= 16, 128 for k <= 32, 64 above, so that
 * the lanes' sorted lists (k slots of a d2 and an int32 each) fit next to the tile. */
#define DPC_KNN_MAX_K 64
#define DPC_KNN_TILE 512
#define DPC_KNN_BLOCK(k) ((k) <= 16 ? 256 : (k) <= 32 ? 128 : 64)

enum {
  DPC_OK = 0,
  DPC_ERR_NULL = -1,        /* a required pointer is NULL */
  DPC_ERR_SHAPE = -2,       /* B, N, D, H, W out of range */
  DPC_ERR_TAPS = -3,        /* tap count even, negative or > DPC_MAX_TAPS */
  DPC_ERR_LDS = -4,         /* an H x W plane does not fit the 160 KiB LDS tile (H*W too large) */
  DPC_ERR_LAUNCH = -5,      /* hipLaunchKernel failed (hipGetLastError has the cause) */
  DPC_ERR_UNSUPPORTED = -6  /* configuration the reference itself cannot run (dead branch) */
};

/* Bits of the optional device status word (DpcParams.status). */
enum {
  DPC_STATUS_BAD_INDEX = 1,   /* a point_index entry was outside [0, N_src): the point was dropped (the reference's fancy
                               * indexing raises IndexError there, dpc/util/point_cloud_to.py:266-295); dpc_densify: a
                               * mesh id out of range or inconsistent, or an edge on more than max_face_count faces;
                               * dpc_render_meshes: a face's vertex index or material id outside its mesh (skipped)    */
  DPC_STATUS_VOXEL_TOO_SMALL = 2, /* dpc_voxel_downsample: open3d's "voxel_size is too small" (nothing was computed)    */
  DPC_STATUS_KEY_OVERFLOW = 4,    /* dpc_voxel_downsample: the batch's voxel keys need more than 64 bits (nothing computed) */
  DPC_STATUS_NONFINITE = 8,       /* dpc_voxel_downsample: a NaN or infinite coordinate (nothing was computed);
                                   * dpc_densify: a non-finite vertex, edge length or midpoint (that model stops);
                                   * dpc_render_points: a non-finite coordinate, colour or radius, or a radius <= 0, in
                                   * a cloud (that image stays background); dpc_render_meshes: a face with a NaN or
                                   * infinite vertex or projection (it was skipped); dpc_fps: a NaN or infinite
                                   * coordinate in a cloud (its indices are -1, its radius2 NaN)                       */
  DPC_STATUS_DENSIFY_ORDER = 16,  /* dpc_densify: a new edge longer than kDnBand x the round's longest edge: the
                                   * round-ordering argument failed and the output may differ from the reference's      */
  DPC_STATUS_NEAR = 32,           /* dpc_render_meshes: a face has a vertex at depth d <= DPC_MESH_NEAR (it was skipped)   */
  DPC_STATUS_EMD_NOT_CONVERGED = 64 /* dpc_emd_fwd: a pair was still unmatched after max_rounds bidding rounds (its emd
                                   * is NaN); DPC_STATUS_BAD_INDEX there and in dpc_fps: the device table differs
                                   * from the host's.  dpc_voxelise: DPC_STATUS_NONFINITE for a NaN or infinite
                                   * coordinate (the point is dropped); DPC_STATUS_BAD_INDEX in the dpc_voxel* entry
                                   * points: a device-table row failed its check (it was not run)                      */
};

/* Geometry and camera constants of one call (dpc/resources/default_config.yaml:77-89 and the cfg fields
 * read at dpc/util/point_cloud_to.py:11-15,128-135; dpc/util/drc.py:52-57,148). */
typedef struct DpcParams {
  int32_t B;               /* clouds in this call (batch_size * step_size * num_candidates)            */
  int32_t N;               /* points per cloud, <= DPC_MAX_POINTS                                       */
  int32_t D, H, W;         /* voxel grid                                                                */
  int32_t taps_xy;         /* length of the x/y Gaussian (odd), 0 = no smoothing (kernel=None / CPU branch) */
  int32_t taps_z;          /* length of the z Gaussian (odd), 0 = no smoothing                          */
  float camera_distance;   /* cfg.camera_distance                                                        */
  float focal_length;      /* cfg.focal_length, used when f == NULL                                      */
  float clip_val;          /* cfg.drc_logsum_clip_val (eps)                                              */
  float max_depth;         /* cfg.max_depth                                                              */
  int32_t point_replicas;  /* R: clouds b*R .. b*R+R-1 share point set b (tf_repeat_0 of the decoded points over views and
                            * pose candidates, dpc/models/model_pc_to.py:302-306) -- then `pc` is [B/R,N,3], read once per
                            * replica instead of being materialised B times, and `dpc` is [B/R,N,3], ZERO-INITIALISED BY
                            * THE CALLER: the replicas' gradients are added into it.  0 or 1: every cloud has its own
                            * points.  Honoured by the fused entry points (dpc_project_*); the stage entry points require
                            * R <= 1. */
  int32_t N_src;           /* points per stored point set when point_index is given (>= 1), otherwise ignored     */
  const int32_t* point_index; /* DEVICE pointer [B,N] int32 | NULL: cloud b projects the points
                            * pc[b/R][point_index[b*N + i]], i < N, of a stored set of N_src points -- every replica
                            * of a point set keeps its own random subset (pc_point_dropout applied after tf_repeat_0,
                            * dpc/models/model_pc_to.py:254-258, 302-306; dpc/util/point_cloud_to.py:269-295) without the
                            * [B,N,3] copies.  Then `pc` is [B/R,N_src,3] and `dpc` is [B/R,N_src,3], ZERO-INITIALISED BY
                            * THE CALLER (the selected points' gradients are added into it; indices may repeat).
                            * An entry outside [0, N_src) never reaches memory: the point is dropped (no contribution, no
                            * gradient) and DPC_STATUS_BAD_INDEX is set in *status when `status` is given.
                            * Honoured by dpc_locate and the fused entry points; the stage entry points require NULL. */
  int32_t* status;         /* DEVICE pointer to one int32 | NULL: DPC_STATUS_* bits are OR-ed into it (never cleared by the
                            * library; the caller zeroes it and reads it at a synchronisation point of its own)           */
  const int32_t* n_live;   /* DEVICE pointer to one int32 | NULL: only the first min(*n_live, N) points of every cloud (of
                            * every point_index row) are live in this call, the rest are skipped without a trace.  N stays the
                            * CAPACITY the buffers and launch grids are sized for -- so a captured HIP graph follows a
                            * scheduled keep-count (dpc/models/model_pc_to.py:68-87, 254-258) from replay to replay.       */
  const float* dev_taps_xy; /* DEVICE pointers to taps_xy / taps_z floats | NULL: when given, the kernels read the tap    */
  const float* dev_taps_z;  /* VALUES from device memory at run time instead of taking them from host_kern_xy / host_kern_z
                            * at launch time.  The host arrays are still required: they select the compiled radius bucket
                            * (dpc_taps_bucket) and must need the same bucket as, or a smaller one than, the device values
                            * ever will.  For captured HIP graphs under a sigma schedule (model_pc_to.py:59-63, 171-179):
                            * dpc_schedule_update rewrites the device values between replays.                              */
} DpcParams;

/* Small per-cloud gradients written by the backward entry points: one buffer of DPC_SMALL_COLS * B floats made of
 * contiguous blocks, so each gradient is a dense tensor of its own: dq [B,4] at float offset DPC_COL_DQ*B,
 * ds [B,1] at DPC_COL_DS*B, dt [B,3] at DPC_COL_DT*B, df [B,1] at DPC_COL_DF*B. */
enum { DPC_COL_DQ = 0, DPC_COL_DS = 4, DPC_COL_DT = 5, DPC_COL_DF = 8, DPC_SMALL_COLS = 12 };

int dpc_abi_version(void);
const char* dpc_strerror(int code);

/* Words of the clamp mask ([B, D, dpc_mask_words_per_plane] uint64; bit i of a plane = voxel y*W+x == i,
 * set where the raw splat value v satisfies 0 <= v <= 1, the pass-through set of torch.clamp's backward). */
size_t dpc_mask_words_per_plane(const DpcParams* p);
/* Binned point records written by the locate kernel and consumed by the slab kernels -- opaque to the caller,
 * dpc_cells_bytes(p) bytes, saved between forward and backward.  Per cloud, ceil(N/256) chunks; each chunk holds
 * its 256 points counting-sorted by z cell: 256 x {int32 code = iz<<20|iy<<10|ix or -1 (out of bounds), 3 x fp32
 * fractional weights encoded so that both r and 1-r keep fp32 relative precision}, 256 x {px, py, pz, int32
 * original point index} sorted alike, (D+2) x uint16 bin offsets (padded to 16 bytes). */
size_t dpc_cells_bytes(const DpcParams* p);
/* First launch of the fused forward on its own: transform (the reference's exact op sequence, see
 * csrc/dpc_common.h) + cell location + per-256-point z sort.  tr_pc [B,N,3] | NULL, cells dpc_cells_bytes(p).
 * Integer/bit-exact against the reference: the parity tests decode `cells` and compare with records computed
 * from the oracle's fp64 tr_pc. */
int dpc_locate(const DpcParams* p, const float* pc, const float* q, const float* t, const float* f, float* tr_pc,
               void* cells, void* stream);
/* Scratch the fused BACKWARD entry points need (one grid-sized fp32 buffer + per-tile partial sums). */
size_t dpc_workspace_bytes(const DpcParams* p);
/* ABI 13.  DPC_OK when the grid of `p` can be served, DPC_ERR_LDS when not: the slab kernels keep whole H x W planes in LDS --
 * one for the forward (planes up to 199 x 199), a cell layer plus its halo for the backward (up to 141 x 141; square 32 / 64 /
 * 128 grids have kernels of their own).  The forward entry points succeed wherever the forward can run; a caller that knows a
 * backward will follow asks with with_backward = 1 and refuses up front (the Python layer does, when gradients are required).
 * The reference takes any vox_size (dpc/util/point_cloud_to.py:11-15); its experiments use 32, 64 and 128. */
int dpc_check_grid(const DpcParams* p, int with_backward);

/* ---------------------------------------------------------------------------------------------------
 * Fused hot path: replaces pointcloud_project_fast (dpc/util/point_cloud_to.py:191-263) =
 * pc_perspective_transform (:118-178) -> pointcloud2voxels3d_fast (:10-87) -> clamp (:201) ->
 * smoothen_voxels3d (:90-103) -> scale+clamp (:218-222) -> drc_projection (dpc/util/drc.py:114-129) ->
 * flip (:242), in three launches (locate + z-sort points -> splat + W/H passes in LDS -> z column pass + DRC).
 *   pc [B,N,3], q [B,4], t [B,3]|NULL, f [B,1]|NULL, s [B,1]|NULL, host_kern_xy[taps_xy], host_kern_z[taps_z]
 *   (HOST pointers: the tap weights travel as kernel arguments)
 * outputs
 *   tr_pc    [B,N,3] (z,y,x) | NULL
 *   cells    dpc_cells_bytes(p) bytes of binned point records (saved for backward)
 *   raw      [B,D,H,W] unclamped splat | NULL (not needed by the backward)
 *   grid_wh  [B,D,H,W] grid after clamp + the W and H passes of the Gaussian (saved for backward, which
 *            recomputes the D pass in registers instead of reading a second grid)
 *   smoothed [B,D,H,W] | NULL: grid after the full Gaussian, before the occupancy scale
 *            (voxels = s ? clamp(s*smoothed,0,1) : smoothed); optional, the hot path does not write it
 *   mask     [B,D,words] uint64 clamp mask (saved for backward)
 *   proj     [B,H,W] silhouette, rows already flipped
 *   trans    [B,H,W] per-ray transmittance prod(1-y) (ray order, not flipped) | NULL; saves the backward a pass
 * ------------------------------------------------------------------------------------------------- */
int dpc_project_fwd(const DpcParams* p, const float* pc, const float* q, const float* t, const float* f,
                    const float* s, const float* host_kern_xy, const float* host_kern_z, float* tr_pc,
                    void* cells, float* raw, float* grid_wh, float* smoothed, uint64_t* mask, float* proj,
                    float* trans, void* stream);

/* Hand-written backward of the chain above (the reference relies on autograd).
 *   dproj    [B,H,W] gradient w.r.t. the (flipped) silhouette
 *   dgrid_wh [B,D,H,W] | NULL: a gradient arriving at grid_wh itself, added in (callers that derive further outputs --
 *            voxels, drc_probs, proj_depth of the reference's output dict -- from the saved grid_wh instead of running the
 *            chain a second time)
 * outputs
 *   dpc    [B,N,3]
 *   dsmall DPC_SMALL_COLS*B floats in the block layout above (ds/dt/df only meaningful when the matching input
 *          was given); fully overwritten, needs no zeroing by the caller. */
int dpc_project_bwd(const DpcParams* p, const float* pc, const float* q, const float* t, const float* f,
                    const float* s, const float* host_kern_xy, const float* host_kern_z, const void* cells,
                    const float* grid_wh, const uint64_t* mask, const float* trans /* from fwd, or NULL */,
                    const float* dproj, const float* dgrid_wh, float* dpc, float* dsmall, void* workspace, void* stream);

/* The same chain with the caller's silhouette loss fused in: the whole of add_proj_loss /
 * proj_loss_pose_candidates (dpc/models/model_pc_to.py:339-385, 410-440), mask pooling and per-view weights included.
 * Cloud b is pose candidate b % K of sample b / K, S = B / K.
 *   gt        [S, f*H, f*W]: the masks (the reference's inputs["masks"], [S,1,Hm,Wm] or [S,Hm,Wm,1]), f = gt_factor >= 1,
 *             f*H and f*W <= 1024 (DPC_ERR_SHAPE otherwise, before any launch).  The kernels pool them where they read a
 *             pixel: gt[s,y,x] = (sum_{i<f} sum_{j<f} masks[s, f*y+i, f*x+j]) / (f*f), summed in fp32 in row-major window
 *             order and divided (not multiplied by the reciprocal) -- ATen's avg_pool2d order, so the pooled values are the
 *             bits of F.avg_pool2d(masks, f) (nn.AvgPool2d(gt_size // pred_size), :346-354).  f = 1: masks already pooled
 *             to the silhouette size (ABI 14's gt).  No pooled copy is ever written.
 *   weights   [S] | NULL: w_s, the reference's inputs["valid_samples"] (cfg.variable_num_views, :432-436); NULL = all ones.
 * Formulas (sse is UNWEIGHTED, as in ABI 14; the selection is unweighted, like the reference's all_loss.argmin):
 *   sse[c]    = sum_pix (gt[c/K] - proj[c])^2
 *   winner[s] = first argmin_k sse[s*K + k]
 *   loss      = sum_s w_s^2 sse[s*K + winner[s]] / S          (w squared: the reference weights the residual, then squares)
 *   d loss / d proj[c] = 2 w_s^2 (proj[c] - gt[s]) / S * dloss for the winner c of sample s, 0 for the others
 * K = 1 is the min-of-1 case of the same formula.  The ray-march kernel accumulates each cloud's sse, a one-block finalize
 * picks the winners and writes the loss.  In the backward d loss / d proj is formed on the fly (never stored) and losing
 * candidates skip all work -- their gradients are exact zeros.  With the column backward fused in (below) the loss is summed
 * in fixed point, so it is the same bits on every run; all-one weights give the bits of weights = NULL, and the weights
 * have no bound (a NaN weight makes the loss NaN).
 *   fwd outputs: proj [B,H,W], trans [B,H,W], sse [B], loss [1], winner [B/K] int32 (+ tr_pc|NULL, cells, grid_wh, mask);
 *                sse_tiles [B, ceil(H*W/256)] scratch: the ray tiles' squared errors, added in tile order by the finalize
 *                launch (no float atomics: sums, winners and loss are the same bits on every run); may be NULL only when
 *                the column backward is fused into the forward (see below), which sums in 64-bit fixed point instead
 *   bwd inputs : dloss = device scalar arriving at `loss` (NULL = 1)
 *
 * Column half of the backward inside the forward (optional): d loss / d proj is linear in dloss, and the forward's
 * ray-march kernel holds each ray's column in registers, so with one candidate per sample (K = 1) it can also run the
 * DRC backward + adjoint D pass for dloss = 1.  Pass bwd_workspace (dpc_workspace_bytes) and bwd_dsmall
 * (DPC_SMALL_COLS*B floats): when the configuration allows it, *column_backward_done is set to 1, the workspace holds
 * dT and the ds partials and bwd_dsmall is zeroed; hand the workspace and the flag to dpc_project_loss_bwd, which then
 * launches the gather kernel only (it multiplies by *dloss).  dpc_project_loss_bwd WRITES dq, ds (and dt, df when t, f
 * are given) into its `dsmall` -- any DPC_SMALL_COLS*B floats, need not be bwd_dsmall; the workspace is left as it was, so
 * the backward may be called again on the same forward.  Pass NULLs / 0 to keep the two halves apart. */
int dpc_project_loss_fwd(const DpcParams* p, const float* pc, const float* q, const float* t, const float* f,
                         const float* s, const float* host_kern_xy, const float* host_kern_z, const float* gt,
                         int gt_factor, const float* weights, int num_candidates, float* tr_pc, void* cells, float* grid_wh,
                         uint64_t* mask, float* proj, float* trans, float* sse, float* sse_tiles, float* loss, int32_t* winner,
                         void* bwd_workspace, float* bwd_dsmall, int* column_backward_done, void* stream);
int dpc_project_loss_bwd(const DpcParams* p, const float* pc, const float* q, const float* t, const float* f,
                         const float* s, const float* host_kern_xy, const float* host_kern_z, const void* cells,
                         const float* grid_wh, const uint64_t* mask, const float* proj, const float* trans,
                         const float* gt, int gt_factor, const float* weights, int num_candidates, const int32_t* winner,
                         const float* dloss, int column_backward_done, float* dpc, float* dsmall, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The whole step in ONE call: dpc_project_loss_fwd followed by dpc_project_loss_bwd -- four launches (one pose candidate per
 * sample: the column backward is fused into the forward) or six (K candidates: locate, slab, ray march, finalize, column
 * backward and gather of the winners) enqueued back to back by native code.  What a training loop calls once
 * per step instead of replaying a captured HIP graph of the two calls: the same kernels, the same results bit for bit, and
 * no graph (on MI355X / ROCm 7.2 the eager native sequence is 2-3 us per step FASTER than the replayed graph: 55.3 against
 * 57.2-58.2 us at B = 32, N = 8000, 64^3; host cost of the call 18 us, well under the GPU time).
 *   gt, gt_factor, weights, num_candidates, trans, sse_tiles, fwd_dsmall, dsmall, workspace, dloss: as in the two calls above
 *   (masks at f times the silhouette's size are pooled inside the kernels: no pooling launch in front of the step; trans and sse_tiles
 *   are needed when the column backward is not fused into the forward, i.e. always for K > 1; may be NULL for K = 1 on the
 *   32/64/128-deep grids).
 * ------------------------------------------------------------------------------------------------- */
int dpc_project_loss_step(const DpcParams* p, const float* pc, const float* q, const float* t, const float* f,
                          const float* s, const float* host_kern_xy, const float* host_kern_z, const float* gt,
                          int gt_factor, const float* weights, int num_candidates, void* cells, float* grid_wh, uint64_t* mask,
                          float* proj, float* trans, float* sse, float* sse_tiles, float* loss, int32_t* winner, void* workspace,
                          float* fwd_dsmall, const float* dloss, float* dpc, float* dsmall, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Stage-level entry points (one per reference function), used for the sub-stage API and to cross-check the
 * fused path.
 * ------------------------------------------------------------------------------------------------- */

/* pc_perspective_transform, quaternion branch (dpc/util/point_cloud_to.py:118-148,169-178;
 * dpc/util/quaternion.py:110-132).  out [B,N,3] in (z,y,x) order. */
int dpc_transform_fwd(const DpcParams* p, const float* pc, const float* q, const float* t, const float* f,
                      float* out, void* stream);
/* dout [B,N,3] -> dpc [B,N,3], dsmall (DPC_SMALL_COLS*B floats, block layout above: dq, dt, df; overwritten). */
int dpc_transform_bwd(const DpcParams* p, const float* pc, const float* q, const float* t, const float* f,
                      const float* dout, float* dpc, float* dsmall, void* stream);

/* pc_point_dropout's random choice (dpc/util/point_cloud_to.py:269-295: np.random.choice(N, n, replace=False) for every
 * cloud) drawn on the device: out [B, n] int32 = for each of B clouds n DISTINCT indices in [0, N), a uniformly random
 * n-subset, ascending.  seed: TWO int64 words in device memory (any values; equal seeds give equal draws) -- they are read
 * by the kernel, so a captured graph whose seed words are refreshed by a captured RNG node draws anew at every replay.
 * The result is what DpcParams.point_index expects.  No host work, no synchronisation. */
int dpc_point_dropout_indices(int B, int N, int n, const int64_t* seed, int32_t* out, void* stream);

/* Schedules under HIP-graph replay (dpc/models/model_pc_to.py:59-87, 171-179, 254-258: sigma_rel(step) and the dropout
 * keep-probability are recomputed every step).  A captured graph freezes kernel ARGUMENTS, so the per-step values live in
 * device memory instead: dev_taps_xy[taps_xy], dev_taps_z[taps_z] (DpcParams.dev_taps_*) and n_live[1] (DpcParams.n_live,
 * the n_live argument of dpc_point_dropout_indices_live).  dpc_schedule_update writes new values with ONE tiny launch on
 * `stream` (the values travel as kernel arguments: no pinned staging buffer, nothing to keep alive); enqueue it in front of
 * every replay.  Any of the three destinations may be NULL.  dpc_taps_bucket: the compiled radius bucket a 1-D kernel needs
 * (after dropping outer taps that cannot change an fp32 result), -1 when it is beyond the fused kernels -- a captured graph
 * stays valid while the bucket of the new taps is <= the bucket it was captured with, and is fastest when equal. */
int dpc_schedule_update(const float* host_kern_xy, int taps_xy, const float* host_kern_z, int taps_z, int n_live,
                        float* dev_taps_xy, float* dev_taps_z, int32_t* dev_n_live, void* stream);
int dpc_taps_bucket(const float* host_kern, int taps);
/* dpc_point_dropout_indices with the keep-count read on the device: rows of `n` slots (the capacity), the first
 * min(*n_live, n) of each filled, ascending.  n_live NULL = n. */
int dpc_point_dropout_indices_live(int B, int N, int n, const int32_t* n_live, const int64_t* seed, int32_t* out, void* stream);

/* pointcloud2voxels3d_fast (dpc/util/point_cloud_to.py:10-87): trilinear scatter of already-transformed
 * points tr [B,N,3] (z,y,x; fp32, or fp64 when tr_is_f64 -- the reference's direct callers pass fp64) into
 * vox [B,D,H,W] (overwritten).  cells (dpc_cells_bytes(p) bytes) is scratch for the point records. */
int dpc_splat_fwd(const DpcParams* p, const void* tr, int tr_is_f64, void* cells, float* vox, void* stream);
/* backward of the scatter: gather dvox [B,D,H,W] at the 8 corners -> dtr [B,N,3] (fp32). */
int dpc_splat_bwd(const DpcParams* p, const void* tr, int tr_is_f64, const float* dvox, float* dtr, void* stream);

/* smoothen_voxels3d (dpc/util/point_cloud_to.py:90-103): zero-padded separable correlation along W, H, D.
 * `transpose` != 0 applies the adjoint (flipped taps), i.e. the backward.  in/out [B,D,H,W]; tmp same size.
 * p->taps_xy == 0 (or p->taps_z == 0) leaves that group of axes alone: the D pass by itself finishes a grid that already
 * went through the W and H passes (the grid_wh of dpc_project_fwd). */
int dpc_smooth(const DpcParams* p, const float* host_kern_xy, const float* host_kern_z, int transpose,
               const float* in, float* out, float* tmp, void* stream);

/* drc_projection / drc_event_probabilities / drc_depth_projection (dpc/util/drc.py:48-129,145-160).
 * vox [B,D,H,W] -> proj [B,H,W] | NULL, probs [D+1,B,H,W] | NULL, depth [B,H,W] | NULL.
 * No row flip here (the reference flips in pointcloud_project_fast, point_cloud_to.py:239-242). */
int dpc_drc_fwd(const DpcParams* p, const float* vox, float* proj, float* probs, float* depth, void* stream);
/* dproj [B,H,W]|NULL, dprobs [D+1,B,H,W]|NULL, ddepth [B,H,W]|NULL -> dvox [B,D,H,W]. */
int dpc_drc_bwd(const DpcParams* p, const float* vox, const float* dproj, const float* dprobs,
                const float* ddepth, float* dvox, void* stream);

/* Caller-side silhouette loss fused with its gradient: add_proj_loss /
 * proj_loss_pose_candidates (dpc/models/model_pc_to.py:339-385, 410-440), the formulas of dpc_project_loss_fwd.
 * gt [S, f*H, f*W] the masks, pooled f x f inside the kernel like there (f = gt_factor >= 1; f > 1 needs f*H, f*W <= 1024;
 * f = 1 reads any [S, H*W]), weights [S] | NULL (= 1), pred [S*K, H*W] the K candidate silhouettes per sample.
 * Per sample the candidate with the smallest (unweighted) sum of squared differences wins (first minimum, like
 * torch.argmin); loss = sum over winners w_s^2 (gt-pred)^2 / S.  Outputs: loss_part [S] (sum them for the loss),
 * winner [S], dpred [S*K, H*W] = d loss / d pred (zero for losing candidates).  ABI 15: gt_factor, weights, and H, W in
 * place of n_pix. */
int dpc_silhouette_loss(const float* gt, int gt_factor, const float* weights, const float* pred, int S, int K, int H, int W,
                        float* loss_part, int32_t* winner, float* dpred, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The exact Gaussian occupancy renderer: pointcloud2voxels of the TF-1 original (dpc/util/point_cloud.py:17-57), the
 * branch of cfg.pc_fast == false (dpc/models/model_pc.py:239-250).  Added without a new ABI number.
 *   c_i = -1 + 2 i / (G-1) (tf.linspace(-1, 1, G): the grid spans [-1,1] although the points live in [-1/2,1/2]),
 *   e_a[n,i] = exp(-(tr[n,a] - c_i)^2 / (2 sigma^2)),  raw[b,z,y,x] = k sum_n e_0[n,z] e_1[n,y] e_2[n,x],  vox = clip(raw, 0, 1)
 * with tr [B,N,3] the transformed points in (z,y,x) order and G = D = H = W.  There is no outlier filter (a point outside
 * the cube adds its tail), no occupancy scale, no translation and no learned focal length on this path.  `normalise`:
 *   DPC_GAUSS_NORM_NONE        k = 1
 *   DPC_GAUSS_NORM_ANALYTICAL  k = 1 / (1.78984352254 (sigma G)^3)                       (pc_normalise_gauss_analytical)
 *   DPC_GAUSS_NORM_PER_POINT   k = 1 and every e_a[n,:] is divided by its own sum over i  (pc_normalise_gauss, which wins)
 * Both directions are fp32 matrix products over the three 1-D tables (csrc/dpc_gauss_voxels.hip): nothing larger than the
 * grid is stored, there is no float atomic, and equal inputs give equal bits on every run.  sigma is a launch argument, so
 * a captured graph cannot follow a sigma schedule on this path.
 * forward:  raw [B,G,G,G] | NULL (the sums before the clip: what the backward takes its pass-through set from; a caller
 *           that wants no gradient passes NULL), vox [B,G,G,G].  N == 0 writes a zero grid.
 * backward: raw as written by the forward, dvox [B,G,G,G] -> dtr [B,N,3]; the pass-through set is the inclusive one of
 *           tf.clip_by_value and torch.clamp, 0 <= raw <= 1.  One launch.  N == 0: nothing to write.
 * DPC_ERR_SHAPE before any launch for D != H or H != W, point_replicas > 1, a point_index, sigma <= 0 or not finite, an
 * unknown `normalise`; DPC_ERR_LDS for G > DPC_GAUSS_MAX_SIDE (the backward keeps three [G,32] tables per wave and two
 * 32 x G tiles of the gradient in LDS); DPC_ERR_NULL for a missing pointer; B == 0 returns DPC_OK with nothing launched.
 * Nothing allocates or synchronises. */
#define DPC_GAUSS_NORM_NONE 0
#define DPC_GAUSS_NORM_ANALYTICAL 1
#define DPC_GAUSS_NORM_PER_POINT 2
#define DPC_GAUSS_MAX_SIDE 64
int dpc_gauss_voxels_fwd(const DpcParams* p, const float* tr, double sigma, int normalise, float* raw, float* vox, void* stream);
int dpc_gauss_voxels_bwd(const DpcParams* p, const float* tr, double sigma, int normalise, const float* raw, const float* dvox,
                         float* dtr, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Ground truth prepared for the losses: cfg.pc_gauss_filter_gt / pc_gauss_filter_gt_rgb of the TF-1 original
 * (gauss_smoothen_image, dpc/util/gauss_kernel.py:14-24; dpc/models/model_pc.py:398-404; dpc/util/losses.py:78-83, 128-129).
 * One launch that resizes the ground truth to the projection's size and blurs it.  Added without a new ABI number.
 *   gt   fp32, S samples of C channels (1 or 3) of Hs x Ws: [S,C,Hs,Ws] when `planar`, else [S,Hs,Ws,C];
 *        Hs = f*H, Ws = f*W for one integer f >= 1, Hs, Ws <= 1024
 *   out  [S,H,W,C] fp32 (overwritten)
 * Per plane, in this order:
 *   remap   where gt == remap_from the value is remap_to (add_proj_depth_loss's max_dataset_depth -> max_depth,
 *           losses.py:121-124); off when remap_from == remap_to
 *   resize  DPC_GT_RESIZE_MEAN: the f x f average, summed row-major in fp32 and divided by f*f (the bits of nn.AvgPool2d(f)
 *           and of dpc_silhouette_loss's pooling); DPC_GT_RESIZE_SAMPLE: g[y,x] = gt[f*y, f*x] (what the depth, colour
 *           and ray-consistency losses read)
 *   blur    tf.nn.depthwise_conv2d twice with padding "SAME": the row pass ([1,ntaps]) first, then the column pass
 *           ([ntaps,1]), the same ntaps taps (odd, <= DPC_MAX_TAPS) for every channel, ZEROS outside the H x W plane (so a
 *           depth map darkens at its border: the reference's behaviour).  Each pass adds its terms in tap order
 *           0..ntaps-1 in fp32, the first a plain product: one tap of 1.0 returns the resized input bit for bit.
 * Taps: dev_taps != NULL -- ntaps floats in DEVICE memory, read by the kernel when it runs (a DeviceSchedule's taps_xy: a
 * captured graph follows sigma); otherwise host_taps, ntaps floats on the host that travel as launch arguments.
 * DPC_ERR_NULL for a missing gt, out, or both tap pointers; DPC_ERR_SHAPE for S <= 0, C not 1 or 3, a non-integer or
 * unequal factor, a source side above 1024, an unknown resize_mode; DPC_ERR_TAPS for an even, non-positive or too long tap
 * count -- all before any launch.  Planes are tiled (16 x 64 outputs and their halo per workgroup, at most 59 KiB of LDS at
 * 63 taps), so no accepted plane is refused for its size: there is no DPC_ERR_LDS here.  No atomics, no host-to-device
 * copy, no synchronisation; safe under graph capture; equal inputs give equal bits. */
#define DPC_GT_RESIZE_MEAN 0
#define DPC_GT_RESIZE_SAMPLE 1
int dpc_gt_smooth(const float* gt, int S, int C, int Hs, int Ws, int planar, int H, int W, int resize_mode, float remap_from,
                  float remap_to, const float* host_taps, const float* dev_taps, int ntaps, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Expected depth and its loss, fused (add_proj_depth_loss, dpc/util/losses.py:113-136, on drc_depth_projection,
 * dpc/util/drc.py:145-160): from grid_wh of dpc_project_fwd (the grid after the clamp and the W, H passes) in one column
 * kernel -- D pass, occupancy scale + clamp, DRC recurrence, depth, squared error -- instead of a smoothed grid, a
 * [D+1,B,H,W] tensor of probabilities and a dozen elementwise passes.  Per ray (b, y, x), v_z the D-pass correlation of
 * grid_wh[b, :, y, x] with the z taps (host_kern_z, or p->dev_taps_z when set; p->taps_z == 0: no pass):
 *   o_z = s ? clamp(s_b v_z, 0, 1) : v_z,   y_z = clamp(o_z, eps, 1 - eps),   A_k = prod_{j<k} (1 - y_j),
 *   p_0 = e^eps y_0,  p_k = y_k A_k,  p_D = e^eps A_D        (dpc_drc_fwd's probabilities),
 *   depth[b, H-1-y, x] = sum_k p_k psi_k,   psi_k = k/D - 1/2 + camera_distance,  psi_D = max_depth   (rows flipped like proj).
 * Loss, one cloud per sample (S = B):
 *   g[s, y, x] = gt_depth[s, f*y, f*x]          TF-1 nearest-neighbour resize without align_corners, f = gt_factor >= 1;
 *   g = max_depth where g == max_dataset_depth  when the two differ (:121-124);
 *   loss = (1/2) sum_s w_s^2 sum_pix (g - depth)^2 / S       tf.nn.l2_loss / num_samples; w = weights [S] | NULL (= 1), squared
 *                                                             like dpc_silhouette_loss's.  The caller applies proj_depth_weight.
 * fwd: gt_depth [S, f*H, f*W] | NULL (projection only: depth alone is written); depth [B,H,W] | NULL; loss_tiles
 *   [B, ceil(H*W/256)] scratch: the ray tiles' squared errors, added in tile order by a one-block second launch (no float
 *   atomics: the loss is the same bits on every run); loss [1].
 * bwd: recomputes the column; the gradient arriving at a ray's depth is dloss w_s^2 (depth - g) / S (dloss: device scalar |
 *   NULL = 1; nothing when gt_depth is NULL) plus ddepth [B,H,W] | NULL (flipped like depth).  Outputs: dgrid_wh [B,D,H,W],
 *   every element overwritten (hand it to dpc_project_bwd's dgrid_wh); ds [B] | NULL, the ray tiles' partials added in tile
 *   order inside the launch (the same bits on every run).  One launch, nothing else is enqueued.
 *   workspace: dpc_depth_workspace_bytes(p) bytes.  Its first 4 * B bytes are the tickets of the in-launch ds reduction:
 *   ZERO ON ENTRY (zeroed by the caller once, when the buffer is made) and zero again when the launch has finished, so one
 *   buffer serves any number of calls that run one after the other (one stream); calls that may overlap need a buffer each.
 *   Only read when ds is given.  The rest is scratch and needs no initialisation.
 * D = 32, 64, 128 with a z kernel of effective radius <= 15 run with the column in registers; every other depth or kernel
 * length takes a generic kernel.  DPC_ERR_SHAPE, before any launch: f < 1, f*H or f*W > 1024, gt_depth without loss or
 * loss_tiles, neither gt_depth nor depth (fwd), neither gt_depth nor ddepth (bwd).  Nothing synchronises or allocates.
 * Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_depth_workspace_bytes(const DpcParams* p);
int dpc_depth_loss_fwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z,
                       const float* gt_depth, int gt_factor, float max_dataset_depth, const float* weights, float* depth,
                       float* loss_tiles, float* loss, void* stream);
int dpc_depth_loss_bwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z,
                       const float* gt_depth, int gt_factor, float max_dataset_depth, const float* weights, const float* dloss,
                       const float* ddepth, float* dgrid_wh, float* ds, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Colour: per-point RGB projected to an image and its loss.  The reference's torch port crashes on this branch
 * (dpc/util/point_cloud_to.py:64, dpc/util/drc.py:137); the definition is its TF-1 original: pointcloud2voxels3d_fast's rgb
 * half (dpc/util/point_cloud.py:98-134), the clips, the division by the occupancies and the flip of pointcloud_project_fast
 * (:244-262, 275-277), project_volume_rgb_integral (dpc/util/drc.py:132-142), add_proj_rgb_loss (dpc/util/losses.py:69-90).
 * The Gaussian between the splat and the integral is dpc_smooth on the [B*3,D,H,W] view of the colour grid (convolve_rgb,
 * point_cloud.py:148-154); the pre-convolution clip is the caller's.  All grids fp32; tr [B,N,3] transformed points (z,y,x),
 * rgb [B,N,3] one row per cloud; colour grids are PLANAR, [B,3,D,H,W].  Stage-level: p->point_replicas <= 1 and
 * p->point_index == NULL (DPC_ERR_SHAPE otherwise).  p->taps_* are not read.
 *
 * dpc_rgb_splat_fwd: out[b, c, iz+k, iy+j, ix+i] += wz[k] wy[j] wx[i] rgb[b,n,c] for every point with all three
 *   coordinates in [-1/2, 1/2], with the cell, the weights and the dropped out-of-range corners of the occupancy splat
 *   (dpc_splat_fwd: the same point record), so a point's colour and occupancy land in the same cells with the same weights.
 *   `out` is zeroed by a launch of the call, then two neighbouring lanes per (cloud, channel, point) add the point's 8
 *   corners, four each (the pair owns the two x corners, neighbours in memory), with fp32 hardware atomics
 *   (global_atomic_add_f32, no compare-and-swap loop).  NOT BIT-REPRODUCIBLE: a voxel's sum depends on
 *   the order its adds arrive in, so two runs on equal inputs may differ in the last bits of the colour grid (and of
 *   everything computed from it); dpc_rgb_splat_fixed_fwd below is the reproducible splat.
 * dpc_rgb_splat_bwd: dC [B,3,D,H,W] -> drgb [B,N,3], drgb_c = sum_corners w dC_c; dtr [B,N,3] | NULL, dpc_splat_bwd's
 *   formula applied to sum_c rgb_c dC_c[corner] (NULL: pc_rgb_stop_points_gradient, point_cloud.py:112-113).  One thread
 *   per point, 24 gathers; no atomics; a point outside the cube gets exact zeros.  Every element is written.
 *
 * dpc_rgb_loss_fwd: per ray (b, y, x), with y_k = clamp(vox[b,k,y,x], eps, 1 - eps), A_k = prod_{j<k} (1 - y_j),
 *   p_0 = e^eps y_0, p_k = y_k A_k, p_D = e^eps A_D (dpc_drc_fwd's probabilities, the product in fp64) and
 *   c_k = C[b,c,k,y,x] / (div[b,k,y,x] + div_eps)  when div is given (pc_rgb_divide_by_occupancies: div is the smoothed RAW
 *         occupancy splat, a constant of the node -- the reference stops its gradient),
 *   c_k = clamp(c_k, 0, 1)                          when clip_after (pc_rgb_clip_after_conv),
 *   proj_rgb[b, H-1-y, x, c] = sum_{k<D} p_k c_k + p_D * 1      (white background; rows flipped like proj).
 *   Loss, one cloud per sample (S = B):
 *     g[s, y, x, c] = gt[s, f*y, f*x, c]      f = gt_factor >= 1: TF-1's bilinear resize_images without align_corners
 *                                             samples exactly at (f*y, f*x) for an integer factor;
 *     loss = (1/2) sum_s w_s^2 sum_{pix,c} (g - proj_rgb)^2 / S       tf.nn.l2_loss / num_samples; w = weights [S] | NULL (= 1),
 *                                                                     squared.  The caller applies proj_rgb_weight.
 *   gt [S,f*H,f*W,3], or [S,3,f*H,f*W] when gt_planar != 0, | NULL (projection only); proj_rgb [B,H,W,3] | NULL;
 *   loss_tiles [B, ceil(H*W/256)] scratch: the ray tiles' squared errors, added in tile order by a one-block second
 *   launch (no float atomics: for one and the same colour grid the loss is the same bits on every run); loss [1].
 * dpc_rgb_loss_bwd: the residual of a ray is r_c = dloss w_s^2 (proj_rgb_c - g_c) / S (dloss: device scalar | NULL = 1;
 *   nothing when gt is NULL; proj_rgb: what the forward wrote, required with gt) plus dproj_rgb [B,H,W,3] | NULL.  Outputs,
 *   every element overwritten: dC [B,3,D,H,W], dC_{c,k} = p_k r_c (times 1 / (div + div_eps), and zero where the after-clip
 *   acted); dvox [B,D,H,W], the DRC backward of dpc_drc_bwd with gp_k = sum_c r_c c_k, gp_D = sum_c r_c:
 *   dL/dy_m = gp_m E_m A_m - (sum_{k>m} gp_k p_k) / (1 - y_m), through the clamp where eps <= vox <= 1 - eps.  The prefix
 *   products are parked in dvox by a first pass down the ray and replaced by a second pass up it: no workspace.  One launch.
 * Any D, one thread per ray.  DPC_ERR_SHAPE, before any launch: gt_factor < 1, f*H or f*W > 1024, gt without loss or
 * loss_tiles, neither gt nor proj_rgb (fwd), neither gt nor dproj_rgb (bwd).  Nothing synchronises or allocates.
 * Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
int dpc_rgb_splat_fwd(const DpcParams* p, const float* tr, const float* rgb, float* out, void* stream);
int dpc_rgb_splat_bwd(const DpcParams* p, const float* tr, const float* rgb, const float* dC, float* drgb, float* dtr,
                      void* stream);
int dpc_rgb_loss_fwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                     const float* gt, int gt_factor, int gt_planar, const float* weights, float* proj_rgb, float* loss_tiles,
                     float* loss, void* stream);
int dpc_rgb_loss_bwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                     const float* gt, int gt_factor, int gt_planar, const float* weights, const float* proj_rgb,
                     const float* dloss, const float* dproj_rgb, float* dvox, float* dC, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Bit-reproducible colour splat that reads shared colour sets in place.  The colour grid of dpc_rgb_splat_fwd with the
 * same cell, weights, dropped corners and fp32 product wz[k] * wy[j] * (wx[i] * c) per contribution, but each contribution
 * is rounded ONCE to signed 64-bit fixed point with 40 fractional bits and added as an integer (64-bit atomic adds into a
 * zeroed [B,3,D,H,W] workspace); a second launch converts the sums to fp32, one rounding in all.  Integer adds commute:
 * the grid -- and everything computed from it -- is the same bits on every run and for every order of a cloud's points.
 *   tr        [B,N,3] transformed points (z,y,x), one row per cloud (outputs' tr_pc);
 *   rgb_sets  [B/R, n_set, 3]: the colour of point i of cloud b is rgb_sets[b / R][point_index ? point_index[b*N + i] : i],
 *             R = p->point_replicas (0 or 1: every cloud has its own set), p->point_index [B,N] int32 | NULL -- the
 *             convention of the fused projection, so the decoder's colours serve all views and dropout rows in place;
 *   n_set     colours per set: p->N without a point_index, p->N_src (>= 1) with one (DPC_ERR_SHAPE otherwise).
 * Range: a colour is accepted when |c| <= 8 -- with weights <= 1 and N <= DPC_MAX_POINTS a voxel's sum then stays below
 * 8 * (2^20 - 1) * 2^40 < 2^63 and cannot wrap.  A colour that is larger, NaN or infinite adds nothing and poisons its
 * CLOUD: every voxel of that cloud's grid is NaN, the other clouds are untouched, the call returns DPC_OK.  A point_index
 * entry outside [0, n_set) never becomes an address: it poisons its cloud likewise and sets DPC_STATUS_BAD_INDEX in
 * *p->status when given.
 * dpc_rgb_splat_fixed_bwd: dC [B,3,D,H,W] -> dtr [B,N,3] | NULL (pc_rgb_stop_points_gradient) with dpc_rgb_splat_bwd's
 *   formulas, one lane per (cloud, point); drgb_sets [B/R, n_set, 3], every element written.  Without sharing (R <= 1, no
 *   point_index) drgb is stored directly and the workspace may be NULL.  With sharing the points' contributions are added
 *   as 64-bit fixed point (2^-40; indices may repeat inside a row) and converted by a second launch: the same bits in any
 *   arrival order.  A contribution that is NaN, infinite or >= 2^20 in magnitude has no fixed-point value: it is not
 *   added and its colour SET's gradient is NaN (one poison word per set), as is the gradient of a set a bad index points into.
 * workspace: dpc_rgb_splat_fixed_workspace_bytes(p, n_set) bytes (0 when the arguments are invalid), 16-byte aligned, no
 *   initialisation needed: 8 bytes per colour voxel plus 4 per cloud for the forward.  The backward touches only the first
 *   8 * 3 * (B/R) * n_set + 4 * (B/R) bytes of it (rounded up to 256), and a buffer of that size is enough for it.
 * DPC_ERR_SHAPE before any launch: p->n_live given (the colour step is not capturable), B % R != 0, n_set as above;
 * DPC_ERR_NULL for a missing pointer.  B == 0: DPC_OK, nothing launched; N == 0: the grid (the gradient) is zeroed.
 * The launches: zero fill, splat, convert (forward); splat backward, and with sharing zero fill and convert (backward).
 * Added without a new ABI number: no existing entry point changed; dpc_rgb_splat_fwd / _bwd keep refusing shared sets.
 * These three are declared with DpcParams' fixed-width types (int32_t = int and uint64_t = size_t on every target of this
 * library, so the calling convention is that of the other entry points): tests/test_rgb_loss_host.py pins the list of
 * `int dpc_rgb_*` prototypes to the four entry points above.
 * ------------------------------------------------------------------------------------------------- */
uint64_t dpc_rgb_splat_fixed_workspace_bytes(const DpcParams* p, int32_t n_set);
int32_t dpc_rgb_splat_fixed_fwd(const DpcParams* p, const float* tr, const float* rgb_sets, int32_t n_set, float* out,
                                void* workspace, void* stream);
int32_t dpc_rgb_splat_fixed_bwd(const DpcParams* p, const float* tr, const float* rgb_sets, int32_t n_set, const float* dC,
                                float* drgb_sets, float* dtr, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Ray-consistency (DRC) losses, fused: the ray potentials sum_k p_k psi_k of the TF-1 original's drc_loss / add_drc_loss and
 * drc_rgb_loss / add_drc_rgb_loss (dpc/util/losses.py:23-66, 93-110) over the probabilities of drc_event_probabilities
 * (dpc/util/drc.py:48-106), without the [D+1,B,H,W] tensor.  One cloud per sample (S = B); p_0 = e^eps y_0, p_k = y_k A_k,
 * p_D = e^eps A_D, A_k = prod_{j<k} (1 - y_j) as above; ray (b, y, x) belongs to image pixel (H-1-y, x); the ground truth is
 * read at (f*row, f*col), f = gt_factor >= 1 (TF-1 resize_images without align_corners, integer factor); w = weights [S] |
 * NULL (= 1), squared like the other losses'.  No 1/2 and no square: the caller applies drc_weight / drc_rgb_weight.
 *
 * Mask loss, from grid_wh of dpc_project_fwd with y_z as in dpc_depth_loss_fwd (D pass with host_kern_z / p->dev_taps_z,
 * occupancy scale s [B] | NULL, clamps):
 *   loss = sum_s w_s^2 sum_rays ((1 - g) sum_{k<D} p_k + g p_D) / S,   g = gt_mask[s, f*row, f*col], gt_mask [S, f*H, f*W].
 *   sum_{k<D} p_k is summed, not taken as 1 - p_D (the e^eps factors: the probabilities do not add up to one).
 * fwd: loss_tiles [B, ceil(H*W/256)] scratch, the ray tiles' costs, added in tile order by a one-block second launch (the
 *   loss is the same bits on every run); loss [1].  Two launches.
 * bwd: recomputes the column; the gradient arriving at every ray's cost is dloss w_s^2 / S (dloss: device scalar | NULL = 1).
 *   Outputs: dgrid_wh [B,D,H,W], every element overwritten; ds [B] | NULL, the tiles' partials added in tile order inside
 *   the launch.  One launch.  workspace: dpc_drc_workspace_bytes(p) bytes with the contract of dpc_depth_loss_bwd's: the first
 *   4 * B bytes are tickets, ZERO ON ENTRY (zeroed by the caller once) and zero again when the launch has finished.
 * D = 32, 64, 128 with a z kernel of effective radius <= 15 run with the column in registers; every other depth or kernel
 * length takes a generic kernel.
 *
 * Colour loss, on the renderer's voxels vox [B,D,H,W] (y_k = clamp(vox, eps, 1 - eps)), the smoothed colour grid C
 * [B,3,D,H,W] and div / div_eps / clip_after as in dpc_rgb_loss_fwd (c_k below is the colour its integral sees):
 *   psi_k = sum_c (g_c - c_{c,k})^2,  psi_D = sum_c (g_c - 1)^2 (white background),  g = gt[s, f*row, f*col, :],
 *   loss = sum_s w_s^2 sum_rays sum_k p_k psi_k / S;     gt [S,f*H,f*W,3], or [S,3,f*H,f*W] when gt_planar != 0.
 * fwd: any D, one thread per ray, two launches (column kernel, one-block finalize); loss_tiles and loss as above.
 * bwd: with r = dloss w_s^2 / S, every element overwritten: dC [B,3,D,H,W], dC_{c,k} = 2 r p_k (c_{c,k} - g_c) (times
 *   1 / (div + div_eps), and zero where the after-clip acted); dvox [B,D,H,W], dL/dy_m = r (psi_m E_m A_m -
 *   (sum_{k>m} psi_k p_k) / (1 - y_m)) through the clamp where eps <= vox <= 1 - eps.  One launch, no workspace: D = 32, 64
 *   keep y and the prefix products in registers (vox, C, div are read once, dvox and dC written once); other depths park the
 *   prefix products in dvox like dpc_rgb_loss_bwd.
 *
 * Return codes as in dpc_depth_loss_* / dpc_rgb_loss_*, before any launch: DPC_ERR_SHAPE for f < 1, f*H or f*W > 1024, a gt
 * without loss or loss_tiles (fwd), p->point_replicas > 1 or p->point_index (colour); DPC_ERR_NULL for a missing grid, gt or
 * output; B == 0: fwd writes a zero loss, bwd does nothing.  Nothing synchronises or allocates.
 * Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_drc_workspace_bytes(const DpcParams* p);
int dpc_drc_loss_fwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_mask,
                     int gt_factor, const float* weights, float* loss_tiles, float* loss, void* stream);
int dpc_drc_loss_bwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_mask,
                     int gt_factor, const float* weights, const float* dloss, float* dgrid_wh, float* ds, void* workspace,
                     void* stream);
int dpc_drc_rgb_loss_fwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                         const float* gt, int gt_factor, int gt_planar, const float* weights, float* loss_tiles, float* loss,
                         void* stream);
int dpc_drc_rgb_loss_bwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                         const float* gt, int gt_factor, int gt_planar, const float* weights, const float* dloss, float* dvox,
                         float* dC, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Evaluation side: point_cloud_distance (dpc/util/point_cloud_distance.py:25-40), the kernel of
 * the Chamfer evaluation (dpc/run/eval_chamfer_to.py:24-44).  For every source point vs[i] ([ns,3]) the nearest target
 * vt[j] ([nt,3]): idx[i] = first j minimising dist = sqrt(sum((vt[j]-vs[i])^2)) (int64, like torch.argmin),
 * min_dist[i] that distance, proj[i] = vt[idx[i]].  fp32, or fp64 when is_f64 (the evaluation runs in fp64); proj,
 * min_dist, idx may each be NULL.  workspace: dpc_nearest_workspace_bytes(ns, nt, is_f64) bytes of scratch.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_nearest_workspace_bytes(int ns, int nt, int is_f64);
int dpc_point_cloud_distance(const void* vs, const void* vt, int ns, int nt, int is_f64, void* proj, void* min_dist,
                             int64_t* idx, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Alignment of unsupervised predictions to the ground truth (dpc/run/compute_alignment.py:28-127: open3d_icp,
 * alignment_to_ground_truth, compute_alignment_candidates): a batched point-to-point ICP with the semantics of open3d
 * 0.9's registration_icp(source, target, max_dist, init, TransformationEstimationPointToPoint(with_scaling=False),
 * ICPConvergenceCriteria(rel_fitness, rel_rmse, max_iter)), all in fp64 (open3d runs in double).
 * src [n_src,3], tgt [n_tgt,3] packed clouds; pair p is (src_start, src_count, tgt_start, tgt_count) = pair_desc[p]
 * (DEVICE) = host_pair_desc[p] (HOST, the same values: the launch geometry is built from it), so pairs may share a target.
 *   start:      the source is transformed by init[p] ([P,4,4] row-major, bottom row taken as 0 0 0 1); T = init; evaluate.
 *   iteration:  estimate update; T = update * T; the stored source points are transformed by update in place and
 *               cumulatively (open3d's pcd.Transform(update)); evaluate.  Stop when |d fitness| < rel_fitness and
 *               |d inlier_rmse| < rel_rmse (strict), or after max_iter updates; the result is the last evaluation and its T.
 *   evaluation: for each source point the nearest target by d2 = (d0*d0 + d1*d1) + d2*d2 (no FMA contraction; exact ties
 *               to the lower index); an inlier when d2 < tau2 (strict), tau2 = max_dist * max_dist formed in fp64 (whether
 *               open3d's FLANN call rounds it to float32 is not checkable here); fitness = n_in / n_src,
 *               inlier_rmse = sqrt(sum d2 / n_in); n_in = 0 gives 0, 0 and the identity update, as open3d does.
 *   estimation: Umeyama without scaling on the inlier pairs (centroids, Sigma = 1/n sum (q-mu_q)(p-mu_p)^T,
 *               R = U diag(1,1,det(U)det(V)) V^T, t = mu_q - R mu_p), solved as Horn's 4x4 quaternion eigenproblem: the
 *               same proper rotation when the singular values are distinct, and finite with det +1 for any n >= 1.
 *   points are moved as x' = ((R00 x + R01 y) + R02 z) + t0 per row, without FMA contraction.
 * Outputs: transform [P,4,4], fitness [P], inlier_rmse [P], iterations [P] (the number of updates applied).  Results are
 * bit-identical from run to run (fixed reduction order, no atomics).  max_iter + 1 rounds are enqueued without any host
 * synchronisation; pairs that have stopped skip their work.  DPC_ERR_SHAPE, before any launch, for max_dist <= 0 or not
 * finite, max_iter < 0, a negative start or count, a range outside [0, n_src) / [0, n_tgt), tgt_count == 0 with
 * src_count > 0.  workspace: dpc_icp_workspace_bytes(pairs, host src counts, host tgt counts) bytes (0 when an argument is
 * invalid).  Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_icp_workspace_bytes(int pairs, const int32_t* src_count, const int32_t* tgt_count);
int dpc_icp_point_to_point(const double* src, int n_src, const double* tgt, int n_tgt, const int32_t* pair_desc,
                           const int32_t* host_pair_desc, int pairs, const double* init, double max_dist, int max_iter,
                           double rel_fitness, double rel_rmse, double* transform, double* fitness, double* inlier_rmse,
                           int32_t* iterations, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Batched Chamfer evaluation (dpc/run/eval_chamfer_to.py:88-145: compute_distance in both directions per view, then
 * np.mean of the float64 distances): P directed nearest-distance problems and their means in one call.
 * pts [n_pts,3] is one packed buffer of all clouds, fp32, or fp64 when is_f64; pair p is (src_start, src_count, tgt_start,
 * tgt_count) = pair_desc[p] (DEVICE) = host_pair_desc[p] (HOST, the same values: the launch geometry is built from it).
 * Sources and targets index the same buffer, so "pred -> GT" and "GT -> pred" are two pairs and views share one GT copy.
 *   distances:  per source point exactly dpc_point_cloud_distance's min_dist and idx (the same scan, the same first-minimum
 *               rule; idx relative to tgt_start, int64);
 *   means:      mean[p] = np.mean of the pair's distances cast to float64, bit for bit: buffers of 8192 elements, each
 *               summed in numpy's pairwise_sum order, the buffer sums added left to right onto 0.0, then an IEEE fp64
 *               divide by src_count; src_count == 0 gives NaN, as np.mean of an empty array does.
 * Outputs: mean [P] float64; min_dist (in the compute type) and idx, each [sum src_count] | NULL, packed in pair order:
 * pair p's points start at sum_{q<p} src_count[q].  No atomics: results are bit-identical from run to run and do not
 * depend on how pairs are batched.  The per-pair prefixes are built on the device from pair_desc: the call copies nothing
 * from the host and can be captured into a hipGraph.  DPC_ERR_SHAPE, before any launch, for pairs < 0, n_pts < 0, a negative
 * start or count, a range outside [0, n_pts), tgt_count == 0 with src_count > 0 (the reference's argmin over an empty set
 * raises), or more than 2^31 - 1 output points.  With valid arguments and NULL device pointers the call returns
 * DPC_ERR_NULL without touching a device, so a binding can validate a table on the host first.  workspace:
 * dpc_chamfer_workspace_bytes(pairs, host_pair_desc, is_f64) bytes (0 when the table is invalid or pairs <= 0).
 * Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_chamfer_workspace_bytes(int pairs, const int32_t* host_pair_desc, int is_f64);
int dpc_nearest_batched(const void* pts, int n_pts, int is_f64, const int32_t* pair_desc, const int32_t* host_pair_desc,
                        int pairs, double* mean, void* min_dist, int64_t* idx, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Chamfer loss: the backward of dpc_nearest_batched, and the means of squared distances.  The reference's
 * point_cloud_distance (dpc/util/point_cloud_distance.py:25-40) is plain torch code and differentiates under autograd;
 * this is its gradient in closed form for P directed pairs at once, with nothing of size Ns x Nt materialised.
 *
 * dpc_nearest_batched_bwd: pts, n_pts, is_f64, pair_desc, host_pair_desc, pairs as in the forward; min_dist, idx
 * [sum src_count] are the forward's outputs for the same points and table.  Upstream gradients: gmean [P] float64 | NULL
 * (of the means) and gdist [sum src_count] in the compute type | NULL (of the per-point values); NULL counts as zeros.
 * For source point i of pair p, with s its coordinates, t = target idx[i] of the pair, d = min_dist[i], n_p = src_count:
 *   weight         w = gdist[i] + gmean[p] / n_p, formed in fp64 and rounded once to the compute type;
 *   distance mode  (squared == 0) the target receives c = ((t - s) / d) * w per component and the source -c: one
 *                  subtraction, one IEEE divide, one multiply, no FMA contraction;
 *   d == 0         (coincident points) the reference's autograd yields NaN (inf * 0).  DELIBERATE DEVIATION: c is exactly
 *                  zero here, for source and target, so a cloud compared with itself has a finite, zero gradient;
 *   squared mode   (squared != 0) the per-point value is d * d (rounded once; its means: dpc_chamfer_pair_means); the
 *                  target receives c = (2 w) * (t - s) and the source -c.  There is no division; min_dist may be NULL;
 *   ties           exact and near ties follow the forward's idx, as the reference's indexing does.
 * dpts [n_pts,3] in the compute type; EVERY row is written, a point in no pair gets zero.  The gradient of packed point
 * x is summed in a fixed order: per pair, the terms x receives as a target are added in ascending source position onto
 * 0.0 (a target nobody chose: +0.0); then, pairs ascending, onto 0.0: the pair's source-role term of x, then the pair's
 * target-role sum of x.  A point may be a source in one pair and a target in others (views share one GT copy; ranges
 * may overlap).  No floating-point atomics: two identical calls are bit-identical, and a pair's contribution does not
 * depend on the other pairs of the call.  The per-pair prefixes are built on the device from pair_desc: no host
 * synchronisation, no host -> device copy, capturable into a hipGraph.  An idx outside [0, tgt_count) (never the
 * forward's own) reads nothing and yields NaN.  DPC_ERR_SHAPE, before any launch, for every table dpc_nearest_batched
 * refuses, and for more than 2^31 - 1 target points summed over the pairs.  With a valid table and NULL device
 * pointers the call returns DPC_ERR_NULL without touching a device.  workspace:
 * dpc_chamfer_bwd_workspace_bytes(pairs, host_pair_desc, is_f64) bytes (0 when the table is invalid or pairs <= 0).
 *
 * dpc_chamfer_pair_means: mean[p] = np.mean, as float64, of the src_count values of pair p in `values` ([sum src_count]
 * in the compute type, packed in pair order), by the summation kernels of dpc_nearest_batched (numpy's order, NaN for an
 * empty pair).  Only the counts of the table are used; the same refusals; workspace: dpc_chamfer_workspace_bytes.
 * Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_chamfer_bwd_workspace_bytes(int pairs, const int32_t* host_pair_desc, int is_f64);
int dpc_nearest_batched_bwd(const void* pts, int n_pts, int is_f64, const int32_t* pair_desc, const int32_t* host_pair_desc,
                            int pairs, const void* min_dist, const int64_t* idx, const double* gmean, const void* gdist,
                            int squared, void* dpts, void* workspace, void* stream);
int dpc_chamfer_pair_means(const void* values, int is_f64, const int32_t* pair_desc, const int32_t* host_pair_desc, int pairs,
                           double* mean, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Batched Earth Mover's Distance: the cost of a one-to-one matching pi between two clouds of n points each, for P pairs
 * in one call, with the matching and a closed-form gradient.  The reference has no EMD; the exact optimum is what
 * scipy.optimize.linear_sum_assignment finds for the same cost matrix, one pair at a time on the host.
 *
 * pred [n_pred,3] and gt [n_gt,3] are packed buffers, fp32, or both fp64 when is_f64; pair p is (pred_start, pred_count,
 * gt_start, gt_count) = pair_desc[p] (DEVICE) = host_pair_desc[p] (HOST, the same values).  The two counts of a pair are
 * equal, n_p in [1, DPC_EMD_MAX_POINTS], and the pairs' ranges ascend without overlap in each buffer: every output is
 * indexed like its input.  All arithmetic is fp64 (fp32 input is widened exactly first), no operation is fused:
 *   d2   = (px-gx)*(px-gx) + (py-gy)*(py-gy) + (pz-gz)*(pz-gz)      the additions left to right
 *   c_ij = d2 (squared != 0) or sqrt(d2)                              the same expression in the bidding and the sum
 * The matching is a forward auction (Bertsekas) with eps-scaling, Jacobi rounds, and THE SCHEDULE IS THE CONTRACT:
 *   span  = max c - min c over the pair;  eps_0 = max(span / 2, eps),  eps_k = max(eps_{k-1} / 5, eps); the phase that
 *           runs with exactly eps is the last.  Prices start at 0 and carry over from phase to phase; every phase starts
 *           with nobody assigned.
 *   round   one snapshot of prices and owners; every unassigned i computes v_ij = -c_ij - price_j, j* = argmax_j v_ij
 *           (ties: the lowest j), v that maximum, w = the maximum over j != j* (v itself when n = 1), and bids
 *           b_i = price_j* + (v - w) + eps_k, the additions left to right.  Every object with bids goes to its highest bid
 *           (ties: the lowest i), its price becomes that bid, and its previous owner becomes unassigned.
 *   a phase ends when nobody is unassigned.  After max_rounds rounds in total a pair that still has rounds to run stops
 *           as not converged.
 * Outputs, for a pair that converged:
 *   emd[p]       (sum_i c_{i,pi(i)}) / n_p, float64: 64 partial sums (terms l, l + 64, ... added in ascending order onto
 *                0.0), then a butterfly over them at distances 32, 16, ... 1; then one IEEE divide.
 *                sum_i c_{i,pi(i)} <= optimum + n_p * eps, so emd exceeds the optimal mean by at most eps (cost units);
 *   assignment   [n_pred] int32: pi(i), an index into the pair's gt points, at row pred_start + i;
 *   inverse      [n_gt] int32: the i with pi(i) = j, at row gt_start + j;
 *   rounds[p]    the bidding rounds it ran, int32.
 * A pair that did not converge has emd NaN, rounds = max_rounds, its unassigned entries -1 (the others are the state
 * it stopped in), and DPC_STATUS_EMD_NOT_CONVERGED is OR-ed into *status (DEVICE int32, zeroed by the caller; NULL
 * allowed).  A NaN coordinate ends there too.  The other pairs of the call are unaffected: a pair's results depend on
 * its own points, eps and max_rounds only, are bit-identical from run to run and do not depend on how pairs are
 * batched (integer LDS max / min resolve the bids; no floating-point atomics).  One workgroup per pair, every loop is
 * bounded by max_rounds, nothing waits on another workgroup.  No host synchronisation and no host -> device copy.
 * DPC_ERR_SHAPE, before any launch, for pairs < 0, n_pred < 0, n_gt < 0, eps <= 0 or not finite, max_rounds < 1, a
 * negative start or count, a range outside its buffer, pred_count != gt_count, a count of 0 or above
 * DPC_EMD_MAX_POINTS, or ranges that do not ascend.  With valid arguments and NULL device pointers the call returns
 * DPC_ERR_NULL without touching a device.  dpc_emd_lds_bytes(n): the LDS a pair of n points takes (0 for n outside
 * [1, DPC_EMD_MAX_POINTS]); there is no workspace, a pair's whole state is in LDS.
 *
 * dpc_emd_bwd: the gradient of sum_p gemd[p] * emd[p] (gemd [P] float64; NULL: zeros) given the forward's emd,
 * assignment and inverse for the same points and table.  With a = pred point i, b = gt point pi(i), w = gemd[p] / n_p,
 * in fp64 and unfused:  squared: c = (2 w) * (a - b);  otherwise c = ((a - b) / d) * w with d = sqrt(d2), and c is
 * exactly zero when d == 0 (coincident points, the rule of dpc_nearest_batched_bwd).  dpred row i = c and dgt row pi(i)
 * = -c, each rounded once to the compute type: both are gathers through the bijection, one thread per point, no atomics.
 * A pair whose emd is NaN gets zero rows.  dpred [n_pred,3] | NULL, dgt [n_gt,3] | NULL: rows inside a pair's range are
 * written, the others are left alone.  The same refusals as the forward.
 * Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_emd_lds_bytes(int n);
int dpc_emd_fwd(const void* pred, int n_pred, const void* gt, int n_gt, int is_f64, const int32_t* pair_desc,
                const int32_t* host_pair_desc, int pairs, int squared, double eps, int max_rounds, double* emd,
                int32_t* assignment, int32_t* inverse, int32_t* rounds, int32_t* status, void* stream);
int dpc_emd_bwd(const void* pred, int n_pred, const void* gt, int n_gt, int is_f64, const int32_t* pair_desc,
                const int32_t* host_pair_desc, int pairs, int squared, const double* emd, const int32_t* assignment,
                const int32_t* inverse, const double* gemd, void* dpred, void* dgt, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Batched farthest-point sampling (FPS): for each of C clouds, `samples` of its points, each the point farthest from
 * everything taken before it.  It brings clouds of unequal size to the common size dpc_emd_fwd needs (the predictions
 * have 8000 points, the ground-truth clouds up to 12647) deterministically and with even coverage.  The reference has
 * no subsampling rule of its own.
 *
 * pts [n_pts,3] is one packed buffer, fp32, or fp64 when is_f64; cloud c is the row (start, count, first, out_start,
 * samples) = cloud_desc[c] (DEVICE, 5 int32) = host_cloud_desc[c] (HOST, the same values): its points are rows
 * [start, start + count) of pts, its outputs rows [out_start, out_start + samples) of indices and radius2.  Input ranges
 * may share or skip rows; output ranges ascend without overlap; 1 <= samples <= count <= DPC_FPS_MAX_POINTS and
 * 0 <= first < count.  All arithmetic is fp64 (fp32 input is widened exactly first), no operation is fused.  For the
 * cloud's points p[0..count):
 *   d2(i,j) = (xi-xj)*(xi-xj) + (yi-yj)*(yi-yj) + (zi-zj)*(zi-zj)      the additions left to right
 *   state:    dist[i] = +inf for all i, nothing taken, cur = first
 *   round k = 0 .. samples-1:
 *     indices[out_start + k] = cur                     int32, an index into the cloud's own points
 *     radius2[out_start + k] = dist[cur]               float64, as it stands BEFORE this round's update: +inf for k = 0,
 *                                                      otherwise the squared distance from the pick to the nearest
 *                                                      earlier pick
 *     cur is taken
 *     for every i not taken: dist[i] = min(dist[i], d2(i, cur))
 *     cur = the i not taken with the largest dist[i]; TIES GO TO THE LOWEST i
 * So the indices of a cloud are distinct, radius2 is non-increasing from k = 1 on, a cloud of coincident points yields
 * first and then the remaining indices in ascending order, and an fp32 cloud yields the indices of the same values
 * stored as fp64.  The arg-max is a maximum over the key (dist, lowest index), dist compared through its bit pattern
 * (non-negative doubles order like integers), merged by compare-and-select across lanes, waves and LDS: no atomics, so
 * results are bit-identical from run to run and do not depend on which clouds share a call.
 * A cloud with a NaN or infinite coordinate has indices -1 and radius2 NaN, and DPC_STATUS_NONFINITE is OR-ed into
 * *status (DEVICE int32, zeroed by the caller; NULL allowed); the other clouds are unaffected.  No entry of the device
 * table becomes an address or a loop bound before it is checked against n_pts, the limits above and the end of the host
 * table's last output range; a device row that fails, or whose size class the host table did not announce, sets
 * DPC_STATUS_BAD_INDEX and is not run (its outputs are left as they were).
 * One workgroup per cloud, every loop is bounded by samples, nothing waits on another workgroup.  No host
 * synchronisation and no host -> device copy: the call can be captured into a hipGraph.  There is no workspace.
 * DPC_ERR_SHAPE, before any launch, for clouds < 0, n_pts < 0, a negative start, a range outside [0, n_pts), a count of
 * 0 or above DPC_FPS_MAX_POINTS, samples outside [1, count], first outside [0, count), a negative out_start, or output
 * ranges that do not ascend (or end beyond 2^31 - 1).  With valid arguments and NULL device pointers the call returns
 * DPC_ERR_NULL without touching a device.  Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
int dpc_fps(const void* pts, int n_pts, int is_f64, const int32_t* cloud_desc, const int32_t* host_cloud_desc, int clouds,
            int32_t* indices, double* radius2, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Voxel-grid evaluation (dpc/util/voxel.py: evaluate_voxel_prediction, voxel2pc): clouds and float grids to bit grids,
 * the five counts of evaluate_voxel_prediction per pair of bit grids, and bit grids back to points.  Every output is
 * integer- or bit-exact: there is one right answer and no tolerance.  The conventions:
 *
 * Grid layout.  A grid is [D,H,W], D = vox_size_z (vox_size when that is -1), H = W = vox_size; point column c goes to
 *   grid axis c, as in pointcloud2voxels3d_fast (point_cloud_to.py:29-30).
 * Voxelisation (the nearest node of the renderer's node-centred grid).  A point is valid iff -0.5 <= p_c <= 0.5 on all
 *   three axes (the reference's outlier filter, :26).  For a valid point, in fp64 (fp32 input is widened exactly first)
 *   and without contraction, t_c = (p_c + 0.5) * (G_c - 1) and its node is i_c = (int)floor(t_c + 0.5): the same node
 *   for an fp32 cloud and its fp64 copy.  Invalid and non-finite points mark nothing and are counted in dropped[cloud];
 *   a NaN or infinite coordinate also ORs DPC_STATUS_NONFINITE into *status.  An index is never formed from an invalid
 *   point.  An empty cloud gives an all-zero grid.
 * Bit grids.  A grid is words = ceil(D*H*W / 32) uint32; voxel f = (d*H + h)*W + w is bit f & 31 of word f >> 5.  The
 *   entry points that write bit grids leave the padding bits of the last word zero; those that read them ignore them.
 * Thresholding a float grid.  occupied = v > threshold, or v >= threshold when `inclusive` (voxel2pc, voxel.py:63, is
 *   exclusive; evaluate_voxel_prediction, :5, inclusive), compared in the grid's own dtype with the threshold rounded to
 *   that dtype (what NumPy 2 does with a Python float; it matters for 0.3 on fp32 grids).  A NaN voxel is unoccupied.
 *   dtype: 0 fp32, 1 fp64, 2 uint8 (a bool grid: occupied = non-zero, threshold and inclusive are not read).
 * The five counts, in evaluate_voxel_prediction's order, each an int64 popcount over a pair (p, g) of bit grids:
 *   diff = |p ^ g|, intersection = |p & g|, union = |p | g|, num_fp = |p & ~g|, num_fn = |~p & g|.
 * voxel2pc keeps the reference's quirk: with x = arange(G) * (1.0 / (G - 1)) + (-0.5) in fp64, nothing fused, and
 *   x[G-1] = 0.5 (np.linspace), voxel (i,j,k) becomes the point (x[j], x[i], x[k]) -- the default 'xy' np.meshgrid swaps
 *   the first two axes -- and points come in ascending flat index (i*G + j)*G + k.  So voxelising the points of
 *   voxel2pc(v, t) gives (v > t) with its first two axes transposed.  Cubic grids with G >= 2 only, as the reference.
 *
 * Limits: 1 <= D, H, W <= DPC_VOXEL_MAX_SIDE.  dpc_voxelise keeps a workgroup's share of a grid's bits in LDS, set by
 * LDS atomic OR and written out by plain stores; by the words of the grid it runs one of three size classes:
 *   1 .. 1024 words (up to 32^3)       the whole grid, 4 KiB, 256 threads
 *   1025 .. 8192 words (up to 64^3)    the whole grid, 32 KiB, 512 threads
 *   above (up to 128^3 = 65536 words)  slabs of 16384 words (2^19 voxels: 32 z-planes at 128^3), 64 KiB, 1024 threads,
 *                                      ceil(words / 16384) workgroups per cloud, each reading the whole cloud
 * Tables: cloud_desc / host_cloud_desc [C,2] int32 (start, count) rows of pts (DEVICE / HOST, the same values; ranges
 * may share rows); pair_desc [P,2] (pred grid, gt grid) indices, so the views of one model share one GT grid; out_desc
 * [B,2] (start, count) rows of xyz per grid, count = what dpc_voxel_count reported, ranges ascending without overlap.
 * A device-table row that fails its check against n_pts / n_pred, n_gt / n_out is not read further, sets
 * DPC_STATUS_BAD_INDEX and leaves its outputs untouched; so does, in dpc_voxel2pc, a count that is not the grid's (no
 * point beyond the row's range is written).  status: DEVICE int32, zeroed by the caller, NULL allowed.
 * Every check runs before any launch (DPC_ERR_SHAPE: a negative size, a side outside the limits, an unknown dtype, a
 * table row outside its array, G < 2 or out ranges that do not ascend in dpc_voxel2pc); valid arguments with NULL
 * device pointers return DPC_ERR_NULL without touching a device; zero items return DPC_OK with nothing launched.  No
 * host synchronisation, no allocation, no workspace, no floating-point atomics and no global atomics but the OR into
 * the status word.  dpc_voxel_unpack writes one byte (0 / 1) per voxel, [B,D,H,W], to a 4-byte aligned `out` (DPC_ERR_SHAPE
 * otherwise).  Added without a new ABI number: no
 * existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
int dpc_voxelise(const void* pts, int n_pts, int is_f64, const int32_t* cloud_desc, const int32_t* host_cloud_desc, int clouds,
                 int D, int H, int W, uint32_t* bits, int32_t* dropped, int32_t* status, void* stream);
int dpc_voxel_threshold(const void* grids, int dtype, int B, int D, int H, int W, double threshold, int inclusive, uint32_t* bits,
                        void* stream);
int dpc_voxel_unpack(const uint32_t* bits, int B, int D, int H, int W, uint8_t* out, void* stream);
int dpc_voxel_stats(const uint32_t* pred_bits, int n_pred, const uint32_t* gt_bits, int n_gt, int D, int H, int W,
                    const int32_t* pair_desc, const int32_t* host_pair_desc, int pairs, int64_t* stats, int32_t* status,
                    void* stream);
int dpc_voxel_count(const uint32_t* bits, int B, int D, int H, int W, int32_t* counts, void* stream);
int dpc_voxel2pc(const uint32_t* bits, int B, int G, const int32_t* out_desc, const int32_t* host_out_desc, int n_out, double* xyz,
                 int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Mesh voxelisation: triangle meshes to solid ground-truth occupancy grids (what the reference expects ready-made as
 * <model>.mat files with a `Volume` array, dpc/run/create_tf_records.py:104-115, made off-line with binvox), for M
 * meshes in one call, and the "carve" fill for any bit grid.  There is no counterpart program in the reference and no
 * binvox to compare with: the rules below are this library's own, tests/mesh_voxels_oracle.py restates them in numpy
 * with every operation written out, and where this text and the oracle could differ in a last bit the oracle is the
 * definition.  Every output is bits; the fp64 arithmetic is elementwise, nothing is fused (csrc/dpc_mesh_voxels.hip).
 *
 * Conventions: those of the voxelisation above, so the grid of a mesh and the grid of a cloud of the same model line up.
 *   Grid [D,H,W], node-centred over [-1/2, 1/2]^3, vertex column c to grid axis c; grid coordinates
 *   u_c = (v_c + 0.5) * (G_c - 1) in fp64 (fp32 vertices widen exactly); bit grids as above; 2 <= D, H, W <=
 *   DPC_VOXEL_MAX_SIDE.
 * Surface.  Node n is set iff the closed cube [n - 1/2, n + 1/2]^3 meets the closed triangle: the 13-axis separating-axis
 *   test (3 box axes, the face normal, 9 edge x axis products) on the vertices translated to the node, p = u - n, with
 *   half-size 0.5; the edges e0 = u1 - u0, e1 = u2 - u1, e2 = u0 - u2 and the normal e0 x e1 are the face's own.  An
 *   axis separates only on a strict inequality, so touching counts.  Candidate nodes: ceil(min_c - 0.5) ..
 *   floor(max_c + 0.5) of the face's bounding box, clamped to the grid.  A zero-area face marks what its edges and points
 *   touch (its normal test never separates).  Geometry outside the cube marks nothing.
 * Fill DPC_MESH_FILL_CARVE.  A node is solid iff on each of the three grid lines through it there is a surface node at
 *   an index <= its own and one at an index >= its own: nothing is removed that cannot be seen from one of the six
 *   axis directions.  Robust to open and self-intersecting meshes; it fills concavities no axis direction sees, by design.
 *   dpc_voxel_carve is the same fill for any bit grids (sides from 1), e.g. the shell of a predicted cloud.
 * Fill DPC_MESH_FILL_PARITY.  Rays along grid axis 0 through the integer (y, x) columns, (y, x) = axes (1, 2).  A face is
 *   projected to (y, x); its edge function of P -> Q at column c is (Q.x - P.x) * (c.y - P.y) - (Q.y - P.y) * (c.x - P.x),
 *   evaluated from the lexicographically smaller endpoint (y first) and negated when that is Q, so two faces sharing an
 *   edge see equal or exactly opposite values.  area = the function of 0 -> 1 at vertex 2; a face with area == 0
 *   contributes nothing; the three values w_k (edge opposite vertex k) and the edge directions are negated when area < 0.
 *   A column is crossed when every w_k > 0, or == 0 on a top-left edge (dy > 0, or dy == 0 and dx < 0), and
 *   (w0 + w1) + w2 != 0.  Depth z* = ((w0 z0 + w1 z1) + w2 z2) / ((w0 + w1) + w2), z the axis-0 grid coordinates; the
 *   crossing toggles plane k = ceil(z*) clamped to [0, D] (k = D reaches no node).  parity = prefix XOR of the toggles
 *   along axis 0; the result is surface | parity.  A column with an odd number of crossings is "open" (it leaks to z = D).
 * Guards.  A face with a vertex that is NaN, infinite or >= DPC_MESH_VOXEL_MAX_COORD in magnitude is skipped and sets
 *   DPC_STATUS_NONFINITE; a face with an index outside [0, count of its mesh's vertices) is skipped and sets
 *   DPC_STATUS_BAD_INDEX: it never becomes an address.  A device-table row that does not lie inside verts / faces sets
 *   DPC_STATUS_BAD_INDEX and its mesh's outputs are left untouched.
 * Arguments of dpc_voxelise_meshes:
 *   verts [n_verts,3] fp32 (is_f64 = 0) or fp64, faces [n_faces,3] int32 with indices local to their mesh, both packed
 *   in mesh order; mesh_desc / host_mesh_desc [M,4] int32 (first vertex, vertices, first face, faces), DEVICE / HOST, the
 *   same values; fill one of DPC_MESH_FILL_*; bits [M, words] the grids; scratch [M, words], needed by
 *   DPC_MESH_FILL_CARVE only (the surface, which the fill reads while it writes bits; NULL otherwise); info [M,2] int32:
 *   (kept faces with a vertex outside the cube, open columns: 0 unless the fill is DPC_MESH_FILL_PARITY); status DEVICE
 *   int32, zeroed by the caller, NULL allowed.  A mesh without faces gives an empty grid.
 * Kernels: one workgroup per (mesh, slab of the grid held in LDS), as dpc_voxelise: bits are OR-ed (toggles XOR-ed) with
 *   LDS atomics and finished words written with plain stores; the result does not depend on the order of the faces and
 *   needs no zeroed output.  A face with many candidate nodes is handed to a whole wave or workgroup.
 * Every check runs before any launch (DPC_ERR_SHAPE: a negative size, a side outside the limits, an unknown fill, a table
 * row outside its array; dpc_voxel_carve: out == bits); valid arguments with NULL device pointers return DPC_ERR_NULL
 * without touching a device; zero items return DPC_OK with nothing launched.  No host synchronisation, no allocation,
 * no floating-point atomics and no global atomics but the OR into the status word.  Added without a new ABI number: no
 * existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
int dpc_voxelise_meshes(const void* verts, int n_verts, int is_f64, const int32_t* faces, int n_faces, const int32_t* mesh_desc,
                        const int32_t* host_mesh_desc, int meshes, int D, int H, int W, int fill, uint32_t* bits, uint32_t* scratch,
                        int32_t* info, int32_t* status, void* stream);
int dpc_voxel_carve(const uint32_t* bits, int B, int D, int H, int W, uint32_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Distance transforms of bit grids: the exact squared Euclidean distance of every voxel to the nearest seed, the surface
 * shell of a grid, and the counts and sums a voxel F-score and a mean surface distance are made of.  There is no
 * counterpart in the reference.  Everything is an integer in index units (voxel spacing 1 on every axis, whatever the
 * grid's sides): there is one right answer and no tolerance.  tests/voxel_edt_oracle.py restates the rules in numpy.
 *
 * Bit grids: those of the voxel-grid evaluation above: [D,H,W], words = ceil(D*H*W / 32) uint32, voxel
 *   f = (d*H + h)*W + w is bit f & 31 of word f >> 5.  Readers ignore the padding bits of the last word, writers leave
 *   them zero.
 * dpc_voxel_edt.  Seeds are the set voxels, or the clear voxels when of_clear is non-zero; padding bits are never seeds, in
 *   either mode.  sq [B,D,H,W] int32: sq[b,d,h,w] = min over the seeds (d',h',w') of grid b of
 *   (d-d')^2 + (h-h')^2 + (w-w')^2, so 0 at a seed; every voxel of a grid without a seed is DPC_VOXEL_EDT_NONE.  Three
 *   separable min-plus passes (csrc/dpc_voxel_edt.hip): along W from the bits, along H, then along D in place on sq, which
 *   is the only buffer between the passes: no workspace and no allocation.
 * dpc_voxel_shell.  out [B, words]: the set voxels with at least one of their six face neighbours clear or outside the
 *   grid.  The padding bits of out are written as zero.  out == bits is refused.
 * dpc_voxel_edt_stats.  sq [n_fields, D,H,W] fields, bits [n_grids, words] grids; pair_desc / host_pair_desc [P,2] int32
 *   rows of (field index, bit-grid index), DEVICE / HOST, the same values, as dpc_voxel_stats takes them (rows may share a
 *   field or a grid); host_thresholds_sq [K] int32 on the HOST, 0 <= K <= DPC_VOXEL_EDT_MAX_THRESHOLDS,
 *   0 <= t_k < DPC_VOXEL_EDT_NONE; out [P, 3 + K] int64 per pair:
 *     n         the set voxels of the bit grid,
 *     reached   those of them whose field value is not DPC_VOXEL_EDT_NONE,
 *     sum_sq    the sum of the field over the reached voxels,
 *     then, per threshold, the count of reached voxels with sq <= t_k.
 *   A device-table row that fails its check against n_fields / n_grids is not read further, sets DPC_STATUS_BAD_INDEX and
 *   leaves its output row untouched.  status: DEVICE int32, zeroed by the caller, NULL allowed.
 *
 * Limits: 1 <= D, H, W <= DPC_VOXEL_MAX_SIDE.  dpc_voxel_edt runs one of three size classes per pass: the plane pass by
 * max(H, W) and the depth pass by D, each <= 32, <= 64 or above.
 * Every check runs before any launch (DPC_ERR_SHAPE: a negative size, a side outside the limits, K out of range, a
 * threshold out of range, a host table row outside its array; dpc_voxel_shell: out == bits); valid arguments with NULL
 * device pointers (or a NULL host table that has rows) return DPC_ERR_NULL without touching a device; zero items return
 * DPC_OK with nothing launched.  No host synchronisation, no allocation, no floating point anywhere and no global atomics
 * but the OR into the status word: a pair's counts and sums leave its workgroup by the stores of one thread.  Added
 * without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
int dpc_voxel_edt(const uint32_t* bits, int B, int D, int H, int W, int of_clear, int32_t* sq, void* stream);
int dpc_voxel_shell(const uint32_t* bits, int B, int D, int H, int W, uint32_t* out, void* stream);
int dpc_voxel_edt_stats(const int32_t* sq, int n_fields, const uint32_t* bits, int n_grids, int D, int H, int W,
                        const int32_t* pair_desc, const int32_t* host_pair_desc, int pairs, const int32_t* host_thresholds_sq, int K,
                        int64_t* out, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Iso-surface extraction (dpc/util/voxel.py: extract_surface): occupancy grids to triangle meshes, for a ragged batch of
 * grids in one call.  The reference calls skimage's Lewiner marching cubes; this is a surface extractor with a stated
 * rule of its own: the same cube-edge vertices, this library's order, no Lewiner interior vertices.  Everything below is
 * exact: there is one right answer and no tolerance.  tests/surface_oracle.py restates the rule in numpy.
 *
 * Grid.  A grid is [D,H,W], fp32 or fp64, sides 1 .. DPC_VOXEL_MAX_SIDE; node (d,h,w) has the flat index
 *   f = (d*H + h)*W + w.  Output column c is grid axis c, as in dpc_voxelise.  Coordinates are in index units (node i is
 *   at i), as skimage with spacing 1.
 * Inside.  A node is inside iff (double)v > iso, strictly, as in voxel2pc; a NaN node is outside.  iso is one double per
 *   grid.
 * Vertices.  The edge from node n to n + e_a (a = 0, 1, 2 for D, H, W) is owned by n and carries a vertex iff exactly one
 *   of its ends is inside.  With va, vb the two values widened to fp64, t = (iso - va) / (vb - va), and the vertex is n
 *   with (double)n_a + t in column a; nothing is fused (csrc/dpc_surface.hip is built with -ffp-contract=off).  A grid's
 *   vertices come in ascending key 3*f(n) + a; a vertex exists once, however many cells use it.
 * Cells.  A cell has corner 0 at node (d,h,w), d < D-1, h < H-1, w < W-1; corner k = 4*dd + 2*dh + dw;
 *   case = sum inside(k) << k.  Cell edge e = 4*a + j runs along axis a; j = u_b + 2*u_c for its offsets on the two other
 *   axes b < c.
 * Triangulation of a case.  On each of the six faces 0, 2 or 4 edges are crossed.  Two crossed edges are joined by a
 *   segment.  Four (the ambiguous face) are joined so that each inside corner of the face is cut off alone: its two
 *   adjacent face edges are joined.  The pairing depends on the face's own four corners only, so two cells sharing a face
 *   agree: the surface is closed.  Each segment is directed so that (v1-v0) x (v2-v0) of the resulting triangles, in
 *   output columns 0, 1, 2, points toward lower values (skimage's default gradient_direction='descent'): a blob above the
 *   level has positive signed volume sum v0 . (v1 x v2) / 6.  The directed segments form disjoint loops; a loop starts at
 *   its lowest edge id, loops are emitted in ascending order of that id, and a loop e0, e1, ... is fanned as
 *   (e0, e_i, e_i+1).  The table is the generated csrc/dpc_surface_table.h (tools/gen_surface_table.py): 256 rows, at most
 *   5 triangles a case, 820 in all.
 * Faces.  A grid's faces come in ascending flat index of the cell's corner 0, then table order; they are int32 indices
 *   into that grid's own vertices, 0-based.  Degenerate triangles (a node exactly at iso is outside and gives t = 0 on
 *   its edges) are kept.
 * Borders and small grids.  Surfaces are open at the grid border.  A grid with a side of 1 has no cell and no face; it
 *   still has the vertices of its crossed edges (the vertex rule does not know about cells).
 * Non-finite values.  A crossed edge with a NaN or infinite end writes its vertex as it comes out (NaN; t = 0 when only
 *   vb is infinite) and ORs DPC_STATUS_NONFINITE into *status (dpc_surface_extract only).  Counts and faces are not
 *   affected.
 *
 * Calling shape, as dpc_voxel_count + dpc_voxel2pc: dpc_surface_count writes counts [B,2] int32 (vertices, faces) per grid;
 * the caller reads them, sizes the outputs and calls dpc_surface_extract with out_desc.
 *   values      the grids' nodes packed one grid after another, n_values of them, fp32 (is_f64 = 0) or fp64
 *   grid_desc / host_grid_desc   [B,4] int32 (first node, D, H, W), DEVICE / HOST, the same values; the grids ascend
 *               in values without overlap (a node has one entry of the workspace's map)
 *   iso         DEVICE double [B]
 *   out_desc / host_out_desc     [B,4] int32 (first vertex row, vertices, first face row, faces), DEVICE / HOST; the counts
 *               are what dpc_surface_count reported, the ranges ascend without overlap
 *   verts       DEVICE double [n_verts,3];  faces  DEVICE int32 [n_faces,3]
 *   workspace   dpc_surface_workspace_bytes(host_grid_desc, B, n_values) bytes (0 for a table the entry points refuse):
 *               8 bytes per tile of 1024 nodes (every grid rounded up to the largest grid's tiles), 4 per grid, 4 per
 *               node; the two passes do not share its contents
 *   status      DEVICE int32, zeroed by the caller, NULL allowed
 * Launches.  dpc_surface_count: k_surface_tiles (per tile of 1024 consecutive nodes the vertices and faces it will emit),
 *   k_surface_scan (one workgroup per grid: the ordered scan over its tiles).  dpc_surface_extract: the same two, then
 *   k_surface_verts (the vertices, and per node an int32 map entry: first vertex id, inside bit, crossing bits) and
 *   k_surface_faces (the faces through the map).  The output order does not depend on scheduling.
 * A device-table row that fails its check against n_values / n_verts / n_faces, or whose out_desc counts are not the
 * grid's, sets DPC_STATUS_BAD_INDEX and nothing of that grid is written; the other grids are unaffected.
 * Every check runs before any launch (DPC_ERR_SHAPE: a negative size, a side outside the limits, a grid outside values or
 * overlapping its predecessor, out ranges that do not ascend, overrun their buffers or exceed 3 vertices a node / 5 faces
 * a cell; the totals are int arguments, so a call's totals fit int32 by construction); valid arguments with NULL device
 * pointers return DPC_ERR_NULL without touching a device; zero grids return DPC_OK with nothing launched.  No host
 * synchronisation inside a call, no allocation, no floating-point atomics and no global atomics but the OR into the
 * status word.  Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_surface_workspace_bytes(const int32_t* host_grid_desc, int B, int n_values);
int dpc_surface_count(const void* values, int n_values, int is_f64, const int32_t* grid_desc, const int32_t* host_grid_desc, int B,
                      const double* iso, int32_t* counts, void* workspace, int32_t* status, void* stream);
int dpc_surface_extract(const void* values, int n_values, int is_f64, const int32_t* grid_desc, const int32_t* host_grid_desc,
                        int B, const double* iso, const int32_t* out_desc, const int32_t* host_out_desc, int n_verts, int n_faces,
                        double* verts, int32_t* faces, void* workspace, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Exact point-to-mesh distance: for n_pairs rows (a range of points, a mesh) in one call, the squared Euclidean distance
 * from every point to the nearest point of the union of the row's closed triangles.  The evaluation measures its
 * distances against sampled ground truth, whose spacing is a floor under every distance; this measures against the
 * surface itself.  There is no counterpart in the reference: the rules below are this library's own,
 * tests/point_mesh_oracle.py restates them in numpy and in exact rational arithmetic.  All arithmetic is fp64 (fp32
 * points and vertices widen exactly first); products and sums may be fused, so a value is right to a few units of
 * 2^-52 S^2, S the largest coordinate magnitude of the row, not to the bit (tests/golden/f28_point_mesh.npz records the
 * bound the tests use).
 *
 * Distance to one face (A, B, C), vertices rotated so that the longest edge lies opposite A:
 *   E0 = B - A, E1 = C - A, E2 = C - B, N = E0 x E1, D = P - A;
 *   (s, t) = the barycentric coordinates of the plane foot point, ((E1.E1) (D.E0) - (E0.E1) (D.E1)) / N.N and
 *   ((E0.E0) (D.E1) - (E0.E1) (D.E0)) / N.N; N.N is the determinant (E0.E0)(E1.E1) - (E0.E1)^2, formed as the squared
 *   length of the cross product; the foot point is inside when N.N > 0, s >= 0, t >= 0 and s + t <= 1, and then
 *   d2 = (D.N)^2 / N.N; otherwise d2 = the least of the three squared distances to the segments AB, AC, BC, each
 *   |R - clamp(R.E / E.E, 0, 1) E|^2 from its first endpoint.
 * Zero-area faces.  A face with two or three coincident vertices, or three collinear ones, is the segment or the point
 *   it degenerates to: the inside test is false when N.N is not > 0 (nothing is divided by it then), and a segment of
 *   zero length takes the parameter 0 (nothing is divided by its length), i.e. it is its first endpoint.
 * Guards.  A face with a vertex that is NaN, infinite or >= DPC_MESH_VOXEL_MAX_COORD in magnitude is skipped and sets
 *   DPC_STATUS_NONFINITE, as in dpc_voxelise_meshes; a face with an index outside [0, vertex_count of its row) is skipped
 *   and sets DPC_STATUS_BAD_INDEX: it never becomes an address.  A row whose faces are all skipped gives +inf for its
 *   points.  A point with such a coordinate gets +inf and sets DPC_STATUS_NONFINITE.  A device-table row that does not
 *   lie inside points / verts / faces sets DPC_STATUS_BAD_INDEX and nothing of it is read or written.
 * Arguments:
 *   points [n_points,3] fp32 (points_f64 = 0) or fp64; verts [n_verts,3] fp32 (verts_f64 = 0) or fp64, independently;
 *   faces [n_faces,3] int32, indices local to the vertex range of their row; pair_desc / host_pair_desc [n_pairs,6]
 *   int32 rows (point_start, point_count, vertex_start, vertex_count, face_start, face_count), DEVICE / HOST, the same
 *   values; several rows may name the same vertex and face ranges (the views of one model share one mesh copy);
 *   d2 [sum point_count] fp64, the rows' points in row order: a row with point_count == 0 writes nothing; workspace
 *   dpc_point_mesh_workspace_bytes(n_pairs) bytes (two int32 prefixes; 0 for n_pairs <= 0); status DEVICE int32, zeroed
 *   by the caller, NULL allowed.
 * Kernels (csrc/dpc_point_mesh.hip): a lane owns a point, a workgroup of DPC_PM_BLOCK lanes stages DPC_PM_FACE_TILE
 *   faces per round in LDS (the per-face terms above are formed once per face there) and every lane walks the tile.  A
 *   call whose point blocks alone would not fill the device splits the face ranges into chunks of whole tiles, at least
 *   DPC_PM_CHUNK_TILES each, over several workgroups; d2 is pre-filled with +inf and every workgroup folds its lanes'
 *   minima in with a 64-bit unsigned atomic min (a non-negative double orders like its bit pattern).  min is exact and
 *   order-free: the result is the same bit for bit however the rows are ordered, batched or split.
 * Every check runs before any launch (DPC_ERR_SHAPE: a negative size, a table row outside its array, face_count == 0 for
 * a row with points, more than 2^31 - 1 output points or work items); valid arguments with NULL device pointers return
 * DPC_ERR_NULL without touching a device; no rows or no points return DPC_OK with nothing launched.  No host
 * synchronisation, no allocation, no floating-point atomics.  Added without a new ABI number: no existing entry point
 * changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_point_mesh_workspace_bytes(int n_pairs);
int dpc_point_mesh_distance(const void* points, int n_points, int points_f64, const void* verts, int n_verts, int verts_f64,
                            const int32_t* faces, int n_faces, const int32_t* pair_desc, const int32_t* host_pair_desc, int n_pairs,
                            double* d2, void* workspace, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Closest points on meshes: dpc_point_mesh_distance with its argmin.  For every point, besides the squared distance, the
 * nearest face of the row's mesh, the closest point Q of that face, Q's weights on the face's vertices and the face's
 * unit normal.  The gradient of the squared point-to-surface distance with respect to the point is 2 (P - Q), so Q is
 * what a surface loss needs (dpc/render/closest.py: point_surface_loss); the normal is what a mesh-based normal
 * consistency needs.  tests/closest_oracle.py restates the rules in numpy and in exact rational arithmetic.
 *
 * The same points, verts, faces, pair_desc / host_pair_desc [n_pairs,6] and guards as dpc_point_mesh_distance.  Per
 * output point (the rows' points in row order, sum point_count of them):
 *   d2       fp64: the squared distance.  The distance to one face is dpc_point_mesh_distance's arithmetic (both kernels
 *            inline the same functions of csrc/dpc_point_mesh.h), so d2 equals that entry point's d2.
 *   face     int32: the index of the nearest face within the row's face range, as the caller numbered it; -1 when the
 *            row has no usable face.  Among faces whose computed d2 are bit-equal the lowest index wins; a skipped face
 *            (its d2 is NaN) never wins.
 *   closest  fp64 [.,3]: Q.  Inside region (the plane foot point lies in the face): Q = P - (D.N / N.N) N.  Otherwise the
 *            point of the nearest of the three segments (the first of equals in the order AB, AC, BC of the staged
 *            rotation -- equal segments meet in the same point): the segment's first endpoint plus t E.  Where a weight
 *            is exactly 1 (t = 0 or t = 1 on any of the segments), Q is that vertex itself, bit for bit.  A zero-area face is the segment or point it degenerates to, so Q lies on that.
 *   weights  fp64 [.,3]: non-negative weights on the three vertices of faces[face] IN THE CALLER'S VERTEX ORDER (not the
 *            staged rotation), summing to 1 up to two roundings, with Q = sum w_k V_k: (1 - s - t, s, t) mapped back
 *            through the rotation in the inside region, (1 - t, t, 0) on the edge's two vertices otherwise.
 *   normal   fp64 [.,3], NULL to skip: (V1 - V0) x (V2 - V0) over its length for the caller's winding of faces[face], every
 *            operation rounded on its own (nothing fused), as numpy's elementwise arithmetic gives it; zeros when that
 *            cross product has no length (a zero-area face).
 * No usable face (every face of the row skipped), or a point with a NaN, infinite or >= DPC_MESH_VOXEL_MAX_COORD
 * coordinate: d2 = +inf, face = -1, closest and weights NaN, normal zero.  The status bits are the ones
 * dpc_point_mesh_distance sets.
 * Kernels (csrc/dpc_closest.hip): dpc_point_mesh_distance's decomposition -- (row, DPC_PM_BLOCK points, chunk of faces)
 *   per workgroup, DPC_PM_FACE_TILE faces staged per round -- with every lane keeping (best, arg) under a strict < while
 *   it walks the faces in ascending order.  There is no atomic: a work item writes its lanes' pairs to its own workspace
 *   slots [chunk][point]; a per-point epilogue reduces the chunks in ascending order with a strict <, stages the winning
 *   face alone and writes the outputs.  The result is the same bit for bit however the faces are cut into tiles and
 *   chunks, however the rows are ordered or batched, and whichever workgroup finishes first.
 * workspace: dpc_point_mesh_closest_workspace_bytes(host_pair_desc, n_pairs) bytes, sized from the host table (three int32
 *   prefixes and 12 bytes per slot; a row has point_count slots per chunk of its faces, one chunk unless the call's point
 *   blocks would not fill the device); 0 for n_pairs <= 0, a NULL table or a table the call would refuse.
 * Every check runs before any launch and returns what dpc_point_mesh_distance returns for the same table (DPC_ERR_SHAPE
 * also for more than 2^31 - 1 slots); valid arguments with NULL device pointers (normal apart) return DPC_ERR_NULL without
 * touching a device; no rows or no points return DPC_OK with nothing launched.  No host synchronisation, no allocation,
 * no atomics but the status word's.  Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_point_mesh_closest_workspace_bytes(const int32_t* host_pair_desc, int n_pairs);
int dpc_point_mesh_closest(const void* points, int n_points, int points_f64, const void* verts, int n_verts, int verts_f64,
                           const int32_t* faces, int n_faces, const int32_t* pair_desc, const int32_t* host_pair_desc, int n_pairs,
                           double* d2, int32_t* face, double* closest, double* weights, double* normal, void* workspace,
                           int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Generalized winding numbers: which side of a mesh a point is on.  w(P) = (1 / 4 pi) sum over the faces of the signed
 * solid angle Omega_f(P) of face f seen from P: 1 inside and 0 outside a closed mesh wound outward, a smooth "how much
 * inside" for a triangle soup (open, self-intersecting, inconsistently closed); no connectivity is used.  There is no
 * counterpart in the reference: the rules below are this library's own, tests/winding_oracle.py restates them in numpy
 * and at 50 digits.  All arithmetic is fp64 (fp32 points and vertices widen exactly first); products and sums may be
 * fused.
 *
 * One face, vertices (V0, V1, V2) in the caller's order, seen from P:
 *   a = V0 - P, b = V1 - P, c = V2 - P;  det = a . (b x c);  den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|;
 *   t = atan2(det, den) / (2 pi) = Omega / 4 pi, in [-1/2, 1/2]; t = 0 when det == 0 (P in the face's plane, P on a
 *   vertex, a zero-area face), whatever the sign of that zero.
 * Fixed-point sum.  Each term is quantised, q = llrint(t 2^DPC_WINDING_FRAC_BITS), the terms of a point are added in
 *   int64, and w = (double)sum 2^-DPC_WINDING_FRAC_BITS.  Integer addition is associative: the result is the same bit for
 *   bit however the faces are cut into tiles and chunks, however the rows are ordered or batched, and whichever workgroup
 *   finishes first.  |q| <= 2^39, so a row with more than 2^22 faces is refused (DPC_ERR_SHAPE).  Away from the
 *   surface a term is right to about 1e-16 against the quantum 2^-40 ~ 9e-13, so a sum is within one quantum per usable
 *   face of the sum of the exactly evaluated, quantised terms.
 * dpc_mesh_winding.  The leading arguments, the table pair_desc / host_pair_desc [n_pairs,6] and the guards of
 *   dpc_point_mesh_distance: a face with a NaN, infinite or >= DPC_MESH_VOXEL_MAX_COORD vertex is skipped (its term is 0)
 *   and sets DPC_STATUS_NONFINITE; a face with an index outside its row's vertices is skipped and sets
 *   DPC_STATUS_BAD_INDEX: it never becomes an address; a point with such a coordinate gets sum 0, w = NaN and
 *   DPC_STATUS_NONFINITE; a device-table row outside its arrays sets DPC_STATUS_BAD_INDEX and nothing of it is read or
 *   written.  sums int64 [sum point_count] and winding fp64 [sum point_count], the rows' points in row order; either may
 *   be NULL, not both.  workspace: dpc_mesh_winding_workspace_bytes(host_pair_desc, n_pairs) bytes, sized from the host
 *   table (three int32 prefixes and 8 bytes per slot; a row has point_count slots per chunk of its faces); 0 for
 *   n_pairs <= 0, a NULL table or a table the call would refuse.
 * dpc_mesh_winding_voxels.  The same sum for the node centres of one [D,H,W] grid per mesh, formed in the kernel (no
 *   [M D H W, 3] array exists anywhere): verts, faces, mesh_desc / host_mesh_desc [meshes,4] as dpc_voxelise_meshes takes
 *   them, 2 <= D, H, W <= DPC_VOXEL_MAX_SIDE; node n of axis c, of G_c nodes, sits at n / (G_c - 1) - 1/2, the division
 *   and the subtraction each rounded on its own: dpc_voxelise_meshes' frame.  bits uint32 [meshes, ceil(D H W / 32)],
 *   dpc_voxelise's layout; every word is written.  A bit is set iff sum > threshold_q, an integer compare
 *   (threshold_q = llrint(threshold 2^40)); a mesh without faces gives an empty grid whatever the threshold.  Face
 *   guards as above; a device-table row outside its arrays sets DPC_STATUS_BAD_INDEX and its words are not written.
 *   workspace: dpc_mesh_winding_voxels_workspace_bytes(host_mesh_desc, meshes, D, H, W) bytes (8 bytes per slot, D H W
 *   slots per mesh and chunk of the largest mesh's faces); 0 for what the call would refuse.  DPC_ERR_SHAPE also for a
 *   mesh of more than 2^22 faces and for more than 2^31 - 1 work items, slots or words.
 * Kernels (csrc/dpc_winding.hip): dpc_point_mesh_distance's decomposition -- a lane owns a point or a node, a workgroup of
 *   DPC_PM_BLOCK lanes stages DPC_PM_FACE_TILE faces per round in LDS, nine doubles a face, widened once there; a call
 *   whose point blocks alone would not fill the device splits the face ranges into chunks of whole tiles, at least
 *   DPC_PM_CHUNK_TILES each.  A work item writes its lanes' partial sums to its own workspace slots [chunk][point]; an
 *   epilogue adds a point's slots and writes the outputs (for a grid: compares and packs the bits).
 * Every check runs before any launch and dpc_mesh_winding returns what dpc_point_mesh_distance returns for the same
 * table (DPC_ERR_SHAPE also for a row of more than 2^22 faces and for more than 2^31 - 1 slots); valid arguments with
 * NULL device pointers return DPC_ERR_NULL without touching a device; nothing to do returns DPC_OK with nothing launched.
 * No host synchronisation, no allocation, no atomics but the status word's.  Added without a new ABI number: no existing
 * entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_mesh_winding_workspace_bytes(const int32_t* host_pair_desc, int n_pairs);
int dpc_mesh_winding(const void* points, int n_points, int points_f64, const void* verts, int n_verts, int verts_f64,
                     const int32_t* faces, int n_faces, const int32_t* pair_desc, const int32_t* host_pair_desc, int n_pairs,
                     int64_t* sums, double* winding, void* workspace, int32_t* status, void* stream);
size_t dpc_mesh_winding_voxels_workspace_bytes(const int32_t* host_mesh_desc, int meshes, int D, int H, int W);
int dpc_mesh_winding_voxels(const void* verts, int n_verts, int is_f64, const int32_t* faces, int n_faces, const int32_t* mesh_desc,
                            const int32_t* host_mesh_desc, int meshes, int D, int H, int W, int64_t threshold_q, uint32_t* bits,
                            void* workspace, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Ray-mesh intersection: what a ray hits first, and how many faces it crosses.  For every ray of a ragged batch of
 * (ray bundle, mesh) rows: the smallest hit parameter t, the face hit there, the hit's weights on that face's vertices,
 * the face's unit normal and the number of faces hit.  Occlusion tests between a viewpoint and surface samples, partial
 * scans and a crossing-parity inside test are built on it (dpc/render/raycast.py).  There is no counterpart in the
 * reference: the rules below are this library's own, tests/raycast_oracle.py restates them in numpy and in exact rational
 * arithmetic.  All arithmetic is fp64 (fp32 rays and vertices widen exactly first) and NOTHING IS FUSED: every product,
 * sum and quotient below is rounded on its own, so numpy's elementwise arithmetic reproduces every bit.
 *
 * Ray.  O + t D; D is NOT normalised, t is in units of |D|: t = 1 is the point O + D.
 * One ray, one face with the vertices (V0, V1, V2) in the caller's order; dot(a, b) = (ax*bx + ay*by) + az*bz and
 * a x b = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx) (Moeller-Trumbore), in this order:
 *   E1 = V1 - V0;  E2 = V2 - V0;  Pv = D x E2;  det = E1 . Pv
 *   no hit when !(fabs(det) > 0)                        (D parallel to the face, a zero-area face, D = 0, a NaN)
 *   T = O - V0;  a = T . Pv;  Q = T x E1;  b = D . Q
 *   s = det > 0 ? 1 : -1;  a' = s*a;  b' = s*b;  m = fabs(det)
 *   inside iff a' >= 0 && b' >= 0 && a' + b' <= m       (inclusive; products only, no division)
 *   with cull_backfaces a face with det < 0 is no hit
 *   t = (E2 . Q) / det;  hit iff inside && t_min <= t && t <= t_max      (both ends inclusive)
 *   u = a / det;  v = b / det;  weights = ((1 - u) - v, u, v) on (V0, V1, V2) in the caller's order
 *   The three IEEE divisions run only for a face the ray is inside of.
 *   This test is not watertight along shared edges and vertices: a ray through an edge may report both faces or, after
 *   rounding, neither.
 * One ray, the faces of its row:
 *   hits     int32, NULL to skip: the number of faces hit (an integer: it does not depend on any order).
 *   t, face  fp64, int32: the smallest t among the hits and its face's index within the row's face range, as the caller
 *            numbered it; among faces whose t are bit-equal the lowest index wins.  A miss: t = +inf, face = -1.
 *   weights  fp64 [.,3]: as above for the face reported; NaN for a miss.
 *   normal   fp64 [.,3], NULL to skip: dpc_point_mesh_closest's normal of faces[face] (each operation rounded on its own,
 *            zeros for a cross product without length); zeros for a miss.
 * Arguments.  origins, directions [n_rays,3], fp64 when rays_f64 else fp32; verts, faces as dpc_point_mesh_distance takes
 *   them; pair_desc / host_pair_desc [n_pairs,6]: (ray_start, ray_count, vert_start, vert_count, face_start, face_count),
 *   the table of dpc_point_mesh_distance with rays for points.  The outputs hold the rows' rays in row order,
 *   sum ray_count of them.  A row with rays and no faces is allowed: every ray misses.
 * Guards.  A face with a vertex that is NaN, infinite or >= DPC_MESH_VOXEL_MAX_COORD in magnitude is skipped and sets
 *   DPC_STATUS_NONFINITE; a face with an index outside its row's vertices is skipped and sets DPC_STATUS_BAD_INDEX: it
 *   never becomes an address.  A ray with such an origin or direction component gets t = NaN, face = -1, hits = 0,
 *   weights NaN, normal zero, and sets DPC_STATUS_NONFINITE.  A device-table row outside the packed arrays sets
 *   DPC_STATUS_BAD_INDEX; nothing of it is read or written.
 * Kernels (csrc/dpc_raycast.hip): dpc_point_mesh_closest's decomposition -- (row, DPC_PM_BLOCK rays, chunk of faces) per
 *   workgroup, a lane owns a ray, DPC_PM_FACE_TILE faces staged per round as (V0, E1, E2), DPC_RAY_LDS_BYTES of LDS --
 *   with every lane keeping (t, face, hits) while it walks the faces in ascending order under a strict <.  A work item
 *   writes its lanes' triples to its own workspace slots [chunk][ray]; a per-ray epilogue reduces the chunks in ascending
 *   order with a strict <, adds the counts, stages the winning face alone and recomputes u, v and the normal with the same
 *   expressions.  The result is the same bit for bit however the faces are cut into tiles and chunks, however the rows
 *   are ordered or batched, and whichever workgroup finishes first.
 * workspace: dpc_ray_mesh_workspace_bytes(host_pair_desc, n_pairs) bytes, sized from the host table (three int32 prefixes
 *   and 16 bytes per slot; a row has ray_count slots per chunk of its faces); 0 for n_pairs <= 0, a NULL table or a table
 *   the call would refuse.
 * Every check runs before any launch: DPC_ERR_SHAPE for a negative size, a table row outside the sizes given, more than
 *   2^31 - 1 rays, work items or slots, a NaN t_min or t_max and t_min > t_max (t_max = +inf is allowed); valid arguments
 *   with NULL device pointers (hits and normal apart) return DPC_ERR_NULL without touching a device; no rows or no rays
 *   return DPC_OK with nothing launched.  No host synchronisation, no allocation, no atomics but the status word's.  Added
 *   without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_ray_mesh_workspace_bytes(const int32_t* host_pair_desc, int n_pairs);
int dpc_ray_mesh_intersect(const void* origins, const void* directions, int n_rays, int rays_f64, const void* verts, int n_verts,
                           int verts_f64, const int32_t* faces, int n_faces, const int32_t* pair_desc, const int32_t* host_pair_desc,
                           int n_pairs, double t_min, double t_max, int cull_backfaces, double* t, int32_t* face, double* weights,
                           int32_t* hits, double* normal, void* workspace, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Batched k-nearest-neighbour search, and surface normals from the neighbours' covariance (PCA): the building blocks of
 * the normal-consistency metric (dpc/render/normals.py).  There is no counterpart in the reference: the rules below are
 * this library's own, tests/normals_oracle.py restates them in numpy.
 *
 * dpc_knn_batched.  Row r = (q_start, q_count, r_start, r_count) names a range of queries and a range of references of
 * the one packed buffer pts [n_pts,3]; a cloud against itself is one row with both ranges the same, and several rows may
 * name one reference range (the views of one model share one GT copy).  T = fp64 when is_f64, else fp32.
 *   distance     for query i and reference j, in T, nothing fused and no square root taken:
 *                d = ref_j - q_i;  d2 = (d0*d0 + d1*d1) + d2*d2   (the expression of dpc_nearest_batched);
 *   neighbours   the k references smallest by the pair (d2, j), in ascending order of that pair: ties in d2 go to the
 *                lower index, inside the list and at its k-th place.  A query is not excluded from its own neighbours
 *                (when queries and references coincide it is normally slot 0, d2 = 0).  A d2 that overflows to +inf is
 *                ordered like any other value;
 *   NaN          a candidate whose d2 is NaN (a NaN coordinate, or inf - inf) never enters a list and ORs
 *                DPC_STATUS_NONFINITE into *status; the other candidates are ranked as without it;
 *   outputs      idx [sum q_count, k] int32, relative to r_start, and d2 [sum q_count, k] in T (NULL: not wanted), the
 *                rows' queries packed in row order; slots beyond r_count, or beyond the candidates that are not NaN, hold
 *                -1 and +inf.  A row with q_count == 0 writes nothing.
 *   The result is the same bit for bit from run to run and however the rows are ordered or batched: a lane owns a
 *   query and walks the row's references in index order; nothing is summed across lanes.
 * dpc_pca_normals.  The same table, and the idx that dpc_knn_batched wrote for it with the same k.  For each query with
 * c valid slots (0 <= idx < r_count), everything in fp64 after exact widening, x_j the neighbours:
 *   mu = (1/c) sum x_j;   C = (1/c) sum (x_j - mu)(x_j - mu)^T, from the deviations (two passes), never from raw moments;
 *   eigenvalues  l0 <= l1 <= l2 of C (c == 0: C counts as the zero matrix), ascending in eigenvalues [sum q_count,3]
 *                (NULL: not wanted), never below zero;
 *   normal       a unit eigenvector of l0, normals [sum q_count,3] fp64; (0, 0, 0) when c < 3 (the eigenvalues are still
 *                those of C).  Where l0 == l1 any unit vector of their eigenspace may be returned;
 *   sign         with viewpoints ([rows,3] fp64, DEVICE): flipped so that n . (viewpoint_r - q_i) >= 0, open3d's
 *                orient_normals_towards_camera_location; without (NULL): the component of largest magnitude is
 *                positive, the lowest axis deciding between equal magnitudes;
 *   guards       an idx value outside [-1, r_count) never becomes an address: it ORs DPC_STATUS_BAD_INDEX into *status
 *                and counts as an invalid slot.
 *   accuracy     is the contract, not the algorithm (a cyclic Jacobi iteration on C / trace C; products and sums may be
 *                fused).  With unit = 2^-52 trace(C) / (l1 - l0): the sine of the angle between the normal and the exact
 *                eigenvector of the exact C is a small multiple of unit, | |n| - 1 | <= 4 2^-52, and every eigenvalue is
 *                within a small multiple of 2^-52 trace(C).  tests/golden/f30_normals.npz records the multiple that
 *                numpy's eigh reaches on the fixtures; the tests allow 8 times it.
 * Both.  row_desc / host_row_desc [rows,4] int32, DEVICE / HOST, the same values; status DEVICE int32, zeroed by the
 * caller, NULL allowed.  A device-table row that does not lie inside pts, or whose outputs do not lie inside what the
 * host table counted, sets DPC_STATUS_BAD_INDEX and nothing of it is read or written.
 * Kernels (csrc/dpc_knn.hip): a lane owns a query; a workgroup of DPC_KNN_BLOCK(k) lanes stages DPC_KNN_TILE references
 * per round in LDS and every lane walks the tile.  Each lane's sorted list lives in LDS as [slot][lane] and its k-th
 * best d2 in a register, so a candidate is rejected with one compare.  LDS per workgroup:
 * DPC_KNN_BLOCK(k) k (sizeof(T) + 4) + 3 DPC_KNN_TILE sizeof(T) bytes, at most 60 KiB: two workgroups per CU in fp64
 * and four in fp32 at every k.  The launch grid is (query blocks of the longest row) x rows; a block sums the q_count of
 * the rows before its own from the device table, so no workspace is needed.
 * Every check runs before any launch (DPC_ERR_SHAPE: k outside [1, DPC_KNN_MAX_K], a negative size, start or count, a
 * range outside [0, n_pts), more than 2^31 - 1 output slots sum q_count x k); valid arguments with NULL device pointers
 * (pts, row_desc, idx; normals too in dpc_pca_normals) return DPC_ERR_NULL without touching a device; no rows or no
 * queries return DPC_OK with nothing launched.  No host synchronisation, no allocation, no workspace, no atomics but
 * the status word.  Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
int dpc_knn_batched(const void* pts, int n_pts, int is_f64, const int32_t* row_desc, const int32_t* host_row_desc, int rows, int k,
                    int32_t* idx, void* d2, int32_t* status, void* stream);
int dpc_pca_normals(const void* pts, int n_pts, int is_f64, const int32_t* row_desc, const int32_t* host_row_desc, int rows, int k,
                    const int32_t* idx, const double* viewpoints, double* normals, double* eigenvalues, int32_t* status,
                    void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Voxel-grid downsampling of ground-truth clouds (densify/downsample_gt.py:47-57: open3d.voxel_down_sample(pcd,
 * voxel_size) per model) for C clouds in one call.  open3d's PointCloud::VoxelDownSample (0.7 - 0.9, the same body in each),
 * restated from its C++ source for one cloud p[0..n), all in fp64 (float32 input is widened exactly first):
 *
 *   vs3  = (vs, vs, vs)
 *   lo   = min_i p[i] - vs3 * 0.5          per component; the min bound of an empty cloud is 0
 *   hi   = max_i p[i] + vs3 * 0.5
 *   refuse if vs <= 0, or vs * 2147483647 < max_c (hi - lo)_c        open3d's two LogError cases
 *   key_i = (int(floor((p[i].x - lo.x) / vs)), ... y ..., ... z ...) subtract, then an IEEE division
 *   for i in input order: acc[key_i] += p[i]; cnt[key_i] += 1      one fp64 add at a time, in input order, from 0.0
 *   out  = { acc[k] / double(cnt[k]) }                             an IEEE division, not a multiply by a reciprocal
 *
 * Output order: open3d emits voxels in its std::unordered_map's iteration order, which is implementation-defined; here
 * it is ascending (kx, ky, kz), lexicographic.  The set of output points is open3d's bit for bit; anything that sums over
 * the points in file order (a Chamfer mean GT -> prediction) can differ in the last bits from an open3d-written file.
 *
 * pts [n_pts,3] is one packed buffer, fp32, or fp64 when is_f64; cloud c is (start, count) = cloud_desc[c] (DEVICE) =
 * host_cloud_desc[c] (HOST, the same values); clouds may share or skip rows.  With M = sum of counts:
 *   out        [M,3] float64 capacity (an upper bound): the voxels of all clouds, packed in cloud order;
 *   out_count  [C] int32, voxels of cloud c; out_offset [C] int32, its first row in out (the exclusive prefix of out_count);
 *   status     one int32 (DEVICE): DPC_STATUS_VOXEL_TOO_SMALL (open3d's refusal, for any cloud), DPC_STATUS_KEY_OVERFLOW
 *              (the keys slot | kx | ky | kz, field widths from the batch's largest cloud index and keys, need more than 64
 *              bits, or a key exceeds 2^31 - 1), DPC_STATUS_NONFINITE (open3d's behaviour for them is undefined) are OR-ed in,
 *              never cleared (the caller zeroes it, as DpcParams.status); when one is set nothing else is computed and
 *              out_count, out_offset are 0.  Read it after a synchronisation of the caller's own.
 * No floating-point atomics: results are bit-identical from run to run and do not depend on how clouds are batched.
 * No host synchronisation and no host -> device copy: the call can be captured into a hipGraph.  DPC_ERR_SHAPE, before
 * any launch, for voxel_size <= 0 or not finite, clouds < 0, n_pts < 0, a negative start or count, a range outside
 * [0, n_pts), or M > 2^31 - 2.  With valid arguments and NULL device pointers the call returns DPC_ERR_NULL without touching
 * a device.  workspace: dpc_downsample_workspace_bytes(C, M) bytes, at most 28 M + 2056 ceil(M / 4096) + 56 C + 2048 (0
 * when an argument is invalid).  Added without a new ABI number: no existing entry point changed.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_downsample_workspace_bytes(int clouds, int members);
int dpc_voxel_downsample(const void* pts, int n_pts, int is_f64, const int32_t* cloud_desc, const int32_t* host_cloud_desc,
                         int clouds, double voxel_size, double* out, int32_t* out_count, int32_t* out_offset,
                         int32_t* status, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Mesh densification of ground-truth models (densify/densify_single.py: parseObj, removeWeirdDuplicate, then densifyN
 * times utils.densify) for `models` ragged meshes in one call, in fp64.  Per model, the reference repeats: pop the live
 * edge e = (lo, hi) first by (length descending, edge index ascending); append the vertex (V[lo] + V[hi]) / 2; append the
 * edges [lo, new] and [hi, new] (the parent's faces, in its slot order); for each face on e, in slot order, append the two
 * sub-faces (hi -> new, then lo -> new) and the median edge [opposite vertex, new] (those two faces).  Lengths are
 * sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) of V[E[0]] - V[E[1]]: np.linalg.norm with numpy's OpenBLAS dot.
 *
 * Inputs are packed; model m's row of model_desc (DEVICE) = host_model_desc (HOST) is 7 int32:
 *   v_start, v_count   rows of verts [n_verts,3] float64 (the parsed vertices);
 *   e_start, e_count   rows of edges [n_edges,2] int32: model-local vertex ids (lo, hi), in the reference's edge order;
 *   f_start, f_count   rows of faces [n_faces,3] int32 (model-local vertex ids, after removeWeirdDuplicate) and of
 *                      face_edges [n_faces,3] int32: the model-local edge opposite vertex j of the face;
 *   budget             splits (the reference's densifyN), >= 0.
 * out [sum(v_count + budget), 3] float64: model m's points start at the exclusive prefix of (v_count + budget): its vertices,
 * then its midpoints in split order (the reference's "points").  max_face_count >= the most faces on any edge.
 *
 * The call enqueues `rounds` rounds (after the set-up when `begin` != 0; the first call of a job has begin = 1, later ones
 * the same arguments with begin = 0).  A round splits, per model, every live edge longer than 0.87 x its longest live edge,
 * in the order above, up to the budget (the new edges are never longer than that).  *active (DEVICE, zeroed by
 * the caller before begin) counts the models with splits left: read it after a synchronisation of the caller's own and
 * enqueue more rounds until it is 0.  status (DEVICE, zeroed by the caller; NULL allowed): DPC_STATUS_BAD_INDEX,
 * DPC_STATUS_NONFINITE (that model is not densified), DPC_STATUS_DENSIFY_ORDER.  No floating-point atomics; results are
 * bit-identical from run to run and do not depend on how models are batched or on the rounds per call.  No host
 * synchronisation and no host -> device copy.  DPC_ERR_SHAPE, before any launch, for negative counts or rounds, a range
 * outside its array, a budget > 0 with no edges, max_face_count outside [0, 2^20], or a model whose output rows, edges
 * (e + n (2 + D)), 3 x faces (3 (f + 2 n D)) or slots (3 f + 4 n D) exceed 2^31 - 1, with D = max(2, max_face_count).  With
 * valid arguments and NULL device pointers it returns DPC_ERR_NULL without touching a device.  workspace:
 * dpc_densify_workspace_bytes(models, sum e_count, sum f_count, sum budget, max_face_count) bytes, at most
 * 72 models + 68 (E + N (2 + D)) + 36 (F + 2 N D) + 4 (3 F + 4 N D) + 512.  Added without a new ABI number.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_densify_workspace_bytes(int models, int64_t edges, int64_t faces, int64_t splits, int max_face_count);
int dpc_densify(const double* verts, int n_verts, const int32_t* edges, int n_edges, const int32_t* faces,
                const int32_t* face_edges, int n_faces, const int32_t* model_desc, const int32_t* host_model_desc,
                int models, int max_face_count, int begin, int rounds, double* out, int32_t* status, int32_t* active,
                void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Point-cloud rendering (dpc/render/render_point_cloud.py:19-53 and render_point_cloud_runner.py: one Blender 2.79b
 * process per model running render_point_cloud_blender.py) for P ragged clouds in one call, ray-traced in fp64.
 *
 * Geometry, after render_point_cloud_blender.py:
 *   points   a prediction-frame point p is the scene point (X, Y, Z) = (p2, -p0, p1) (add_points, :150-164: is_mvc
 *            negates column 0, then x = p[2], y = p[0], z = p[1]); the caller maps them, this call takes scene points.
 *            Each is a sphere of radius point_size = 0.01, DEFAULT_SIZE times the unit UV-sphere prototype (:113, :137,
 *            :196); per-point radii replace it (load_data's colored subsets, :139-147).
 *   camera   obj_centened_camera_pos(d, az, el) = (d cos az cos el, d sin az cos el, d sin el) (deg / 180 * pi), placed
 *            at C = (y, x, z) (the swap at :46-48); TRACK_NEGATIVE_Z / UP_Y on the origin: f = -C / |C|,
 *            r = normalise(f x e_z), u = r x f.  Elevation +-90 deg (|f x e_z| < 1e-12) has no such frame: the Python
 *            layer refuses it.  Frames are computed on the host in fp64 and passed per image: no device trigonometry.
 *   lens     F = lens_mm / 32 * S pixels for an S x S image (32 mm sensor).  like_train_data (:83-87) sets 60 mm,
 *            F = 1.875 S, the training renderer's focal_length; without it Blender keeps its startup camera (35 mm in
 *            2.79's default scene, not checked here).
 *   samples  pixel (i, j) (row i from the top) has ss x ss samples (a, b):
 *              x_s = (j + (b + 0.5) / ss) - S/2,   y_s = S/2 - (i + (a + 0.5) / ss),
 *              D = (f + (x_s / F) r) + (y_s / F) u, per component in that order.
 *   hit      m = C - P, a = D.D, b = m.D, c = m.m - r^2, disc = b b - a c; the sphere is hit when c > 0, disc >= 0 and
 *            t = (-b - sqrt(disc)) / a > 0.  Each sample keeps the minimum of the 64-bit key (bits(float32(t)) << 32) | k,
 *            k the point's index in its cloud: ties in float32 depth go to the lowest index; none: background (-1).
 *   shading  (our own; Cycles is not reproduced) at the winner, with the fp64 t: H = C + t D, n = (H - P) / r,
 *            v = -D / |D|, colour = albedo (0.4 + 0.6 max(0, n.v)), albedo 0.5 grey (the prototype material, :95-97)
 *            or the point's colour; background white (horizon_color = (1, 1, 1), :64).
 *   pixel    the ss^2 sample colours summed in fp64 in row-major (a, b) order onto 0.0, divided once by ss^2 and rounded
 *            once to float32.  (The uint8 image, floor(255 clip(v, 0, 1) + 0.5) of that float32, is the Python layer's.)
 * All of it in fp64 with every operation rounded on its own (built with -ffp-contract=off); dot products are
 * (x x' + y y') + z z'; sqrt and division are the correctly rounded IEEE operations.
 *
 * Deliberate deviations from the reference's image: exact spheres instead of bevelled UV spheres; no round trip of the
 * coordinates through the PLY text's '%f'; a box filter over stratified samples instead of Cycles' path tracing and pixel
 * filter; no colour management; RGB without an alpha channel.
 *
 * Arguments: points [n_points,3] float64 (DEVICE), scene frame; colors [n_points,3] float32 (DEVICE) or NULL (grey);
 * radii [n_points] float64 (DEVICE) or NULL (every point `radius`); cloud p is (start, count) = table[p] (DEVICE) =
 * host_table[p] (HOST, the same values), k counting from start; frames [P,12] float64 (DEVICE): C, r, u, f of image p;
 * image_size S, supersample ss, focal F (pixels), radius the default radius.  Outputs: image [P,S,S,3] float32 (DEVICE);
 * ids [P,S ss,S ss] int32 (DEVICE) or NULL: the winning k of every sample (row i ss + a, column j ss + b), -1 for none.
 * status (DEVICE, zeroed by the caller; NULL allowed): DPC_STATUS_NONFINITE when a point of a cloud has a NaN or infinite
 * coordinate, colour or radius, or a radius that is not > 0; that image (and its ids) stays background.  No
 * floating-point atomics: the per-sample minimum is an integer one, so results are bit-identical from run to run and do
 * not depend on how clouds are batched.  No workspace, no host synchronisation and no host -> device copy.
 * DPC_ERR_SHAPE, before any launch, for P < 0, n_points < 0 or 3 n_points > 2^31 - 1, S outside [1, 4096], ss outside
 * [1, 4], F or radius not finite and > 0, a negative start or count, a range outside [0, n_points), or
 * P ceil(S / 16)^2 x 256 > 2^31 - 1 (the launch's work-items).  With valid arguments and NULL device pointers it returns
 * DPC_ERR_NULL without touching a device.  Added without a new ABI number.
 * ------------------------------------------------------------------------------------------------- */
int dpc_render_points(const double* points, const float* colors, const double* radii, int n_points, const int32_t* table,
                      const int32_t* host_table, int images, const double* frames, int image_size, int supersample,
                      double focal, double radius, float* image, int32_t* ids, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Training views from triangle meshes: what the reference downloads as <synth_set>-renders.tar.gz (render_N.png RGBA,
 * depth_N.png, camera_N.mat per model, made with Blender) for W views of M ragged meshes in one call, rasterised in fp64
 * with the camera of the reference's own projection (pc_perspective_transform, dpc/util/point_cloud_to.py:136-178).
 *
 *   camera   view w has a rotation R (row-major 3 x 3: the rotation of q = quaternion_from_campos(cam_pos), computed on
 *            the host in fp64), camera_distance and focal_length f.  A vertex p (.obj coordinates) goes to
 *              r_k = (R_k0 p_0 + R_k1 p_1) + R_k2 p_2,   d = r_0 + camera_distance,   v = (r_1 f) / d,   u = (r_2 f) / d,
 *            and to the pixel coordinates  x = (u + 0.5) S  (columns),  y = (0.5 - v) S  (rows, row 0 at v = +0.5).
 *            Pixel (i, j) of the S x S image covers y in [i, i + 1), x in [j, j + 1).
 *   samples  ss x ss per pixel: sample (a, b) of pixel (i, j) at y = i + (a + 0.5) / ss, x = j + (b + 0.5) / ss.
 *   coverage the edge function of the directed edge a -> b at p is E = (b_x - a_x)(p_y - a_y) - (b_y - a_y)(p_x - a_x),
 *            evaluated with the ends in lexicographic (x, then y) order and negated when that swapped them, so that the
 *            two faces on an edge get the same bits.  With e_0, e_1, e_2 the functions of the edges 1 -> 2, 2 -> 0, 0 -> 1
 *            and A that of 0 -> 1 at vertex 2, a sample is inside when A != 0 and all e_k >= 0 or all e_k <= 0
 *            (inclusive, both windings).  A projected triangle with A = 0 covers nothing.
 *   depth    perspective-correct: 1 / d = ((e_0 / A) w_0 + (e_1 / A) w_1) + (e_2 / A) w_2 with w_k = 1 / d_k; a sample
 *            whose 1 / d is not > 0 is not covered.
 *   visible  each sample keeps the minimum of the 64-bit key (bits(float32(d)) << 32) | k, k the face's index in its mesh,
 *            an integer minimum: the image does not depend on the order of the faces, on tiling or on batching, and
 *            ties in float32 depth go to the lowest index.
 *   guards   a face with a vertex index outside its mesh or a material id outside its table (DPC_STATUS_BAD_INDEX), with
 *            a vertex whose coordinates, d, x or y are not finite (DPC_STATUS_NONFINITE) or with a vertex at
 *            d <= DPC_MESH_NEAR (DPC_STATUS_NEAR; a guard, not a clipping path: ShapeNet models sit inside the unit
 *            cube at distance 2) is skipped whole and sets its bit.  None of these values becomes an address.
 *   shading  per covered sample Kd[material] (DPC_MESH_AMBIENT + DPC_MESH_DIFFUSE |n_0| / |n|), n = (r_1 - r_0) x
 *            (r_2 - r_0) the face normal in camera space (|n| = 0: the ambient term alone): a headlight along the view
 *            axis (-1, 0, 0).  No textures, no smooth normals, no shadows, no specular term.
 *   pixel    alpha = covered / ss^2; rgb = the covered samples' colours summed in row-major (a, b) order onto 0.0 and
 *            divided by their number, clipped to [0, 1] (straight alpha; 0 when nothing is covered); every channel to
 *            uint8 by floor(255 x + 0.5).
 *   depth px the fp64 d of the sample with the smallest key of the pixel (the first such sample in (a, b) order), stored
 *            as min(65535, floor(d / 10 * 65535 + 0.5)): the inverse of the reference's loadDepth
 *            (dpc/run/create_data_torch.py:66-70); 65535 where nothing is covered.  face_id is that key's face, -1 for none.
 * All of it in fp64 with every operation rounded on its own (built with -ffp-contract=off); sqrt and division are the
 * correctly rounded IEEE operations.
 *
 * Deliberate deviations from the archive's Blender renders: flat shading by a headlight instead of Blender's lamps and
 * smooth normals; diffuse colour only (no textures, no transparency); a box filter over a regular sample grid.
 * dpc_render_meshes_shaded below adds the models' textures and smooth normals.
 *
 * Arguments: verts [n_verts,3] float64, faces [n_faces,3] int32 (vertex indices local to the mesh), face_mat [n_faces] int32
 * (local to the mesh's materials), kd [n_mats,3] float64 (all DEVICE); mesh m is the row meshes[m] (DEVICE) =
 * host_meshes[m] (HOST, the same values) of 6 int32: (vertex start, count, face start, count, material start, count);
 * view w renders mesh view_mesh[w] (DEVICE) = host_view_mesh[w] (HOST) with view_cam[w] (DEVICE) = 11 float64: R,
 * camera_distance, focal_length.  Several views may share a mesh.  Outputs (DEVICE): rgba [W,S,S,4] uint8, depth [W,S,S]
 * uint16, face_id [W,S,S] int32 or NULL.  status (DEVICE, zeroed by the caller; NULL allowed) gets the bits above OR-ed in.
 * workspace (DEVICE): dpc_render_meshes_workspace_bytes(host_meshes, M, host_view_mesh, W) bytes (0 for a table it
 * refuses), 16 W + 32 (vertices of the views' meshes) + 8 (faces of the views' meshes) + 4 * 15 at most.  No
 * floating-point atomics, no allocation, no host synchronisation and no host -> device copy.  DPC_ERR_SHAPE, before any
 * launch, for negative counts, 3 n > 2^31 - 1, S outside [1, 1024], ss outside [1, 4], W > 65535, a negative start or
 * count or a range outside its buffer, a view's mesh outside [0, M), or W ceil(S / 16)^2 x 256 > 2^31 - 1.  With valid
 * arguments and NULL device pointers it returns DPC_ERR_NULL without touching a device.  Added without a new ABI number.
 * ------------------------------------------------------------------------------------------------- */
#define DPC_MESH_NEAR 1e-3    /* the near guard: faces with a vertex at d <= this are skipped */
#define DPC_MESH_AMBIENT 0.25 /* shading: ambient + diffuse = 1 */
#define DPC_MESH_DIFFUSE 0.75
size_t dpc_render_meshes_workspace_bytes(const int32_t* host_meshes, int n_meshes, const int32_t* host_view_mesh, int views);
int dpc_render_meshes(const double* verts, int n_verts, const int32_t* faces, const int32_t* face_mat, int n_faces,
                      const double* kd, int n_mats, const int32_t* meshes, const int32_t* host_meshes, int n_meshes,
                      const int32_t* view_mesh, const int32_t* host_view_mesh, const double* view_cam, int views,
                      int image_size, int supersample, uint8_t* rgba, uint16_t* depth, int32_t* face_id,
                      int32_t* status, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The same views with the models' own textures (map_Kd) and smooth vertex normals (vn): dpc_render_meshes with
 * per-corner attributes interpolated perspective-correctly over the winning face of every sample.  Camera, samples,
 * coverage, depth, the visible face, the guards, the pixel filter, depth px and face_id are dpc_render_meshes's, by the
 * same code: for the same meshes and cameras depth, face_id and the alpha channel are its bytes.  Only the colour of a
 * covered sample differs.  For the sample's winning face, with e_k, A and w_k as above:
 *
 *   weights  g_k = (e_k / A) w_k,   d = 1 / ((g_0 + g_1) + g_2)  (the sample's fp64 depth),   c_k = g_k d.
 *   texture  the face is textured when mat_tex[material] >= 0 and its three face_uv entries are >= 0.  Then
 *              u = (c_0 u_0 + c_1 u_1) + c_2 u_2,   v likewise,   fu = u - floor(u),   fv = v - floor(v)   (repeat),
 *              x = fu Wt - 0.5,   y = (1 - fv) Ht - 0.5   (row 0 of the image is the top of the texture, v = 1),
 *              x0 = floor(x), ax = x - x0, bx = 1 - ax;   y0 = floor(y), ay = y - y0, by = 1 - ay,
 *            the integer columns x0, x0 + 1 and rows y0, y0 + 1 wrapped modulo Wt and Ht, a texel T = byte / 255.0, and
 *              rgb = (T[y0][x0] bx + T[y0][x0 + 1] ax) by + (T[y0 + 1][x0] bx + T[y0 + 1][x0 + 1] ax) ay
 *            per channel takes the place of Kd[material].  No colour-space conversion, no alpha, no map_d, no
 *            mip-mapping.  An untextured face, and a sample whose u or v is not finite, use Kd[material].
 *   normals  when the face's three face_vn entries are >= 0: m_k = R vn_k ((R_q0 p_0 + R_q1 p_1) + R_q2 p_2, not
 *            normalised), n = (c_0 m_0 + c_1 m_1) + c_2 m_2 per component, |n| = sqrt((n_0^2 + n_1^2) + n_2^2) and
 *            shade = DPC_MESH_AMBIENT + DPC_MESH_DIFFUSE (|n_0| / |n|).  When |n| is zero or not finite, or the face
 *            lacks a normal at a corner, shade is dpc_render_meshes's face-normal shade.
 *   colour   the sample's colour is rgb shade (one product per channel); pixels as in dpc_render_meshes.
 *   guards   besides dpc_render_meshes's: a face_uv or face_vn entry below -1 or outside the mesh's range, or a
 *            mat_tex of the face's material below -1 or outside the mesh's textures, is DPC_STATUS_BAD_INDEX; a uv or a
 *            normal that the face names (entry >= 0) and that is not finite is DPC_STATUS_NONFINITE; the face is skipped
 *            whole.  None of these values becomes an address; texel addresses come from the wrapped integers alone.
 * Every product, sum, division, floor and sqrt is one rounded fp64 operation (-ffp-contract=off).
 *
 * Remaining deviations from the archive's Blender renders: a headlight only; no shadows or specular term; no
 * transparency; no mip-mapping; no colour management; a box filter over a regular sample grid.
 *
 * Arguments: dpc_render_meshes's, and uv [n_uv,2] float64, face_uv [n_faces,3] int32 (local to the mesh's uvs, -1: none),
 * normals [n_vn,3] float64, face_vn [n_faces,3] int32 (local, -1: none), mat_tex [n_mats] int32 (the material's texture,
 * local to the mesh's textures, -1: none), texels: n_texel_bytes uint8 of packed RGB rows (all DEVICE); texture t is the
 * row tex[t] (DEVICE) = host_tex[t] (HOST) of 3 int64: (byte offset of its first texel, width, height), offsets beyond
 * 2^31 allowed.  A mesh row has 12 int32: dpc_render_meshes's 6, then (uv start, count, normal start, count, texture
 * start, count).  face_uv NULL switches textures off (uv, mat_tex, tex and texels are then not read), face_vn NULL smooth
 * normals; with both NULL, or with every face_uv, face_vn or mat_tex entry -1, the output is dpc_render_meshes's byte for
 * byte.  workspace: dpc_render_meshes_shaded_workspace_bytes(host_meshes (rows of 12), M, host_view_mesh, W) bytes, the
 * same figure as dpc_render_meshes's: attributes are fetched per face where a pixel is shaded.  No floating-point
 * atomics, no allocation, no host synchronisation and no host -> device copy.  DPC_ERR_SHAPE, before any launch, for
 * everything dpc_render_meshes refuses, and for n_uv, n_vn, n_tex or n_texel_bytes < 0, 2 n_uv or 3 n_vn > 2^31 - 1, a
 * uv, normal or texture range outside its buffer, a texture with a negative offset, a side outside [1, 65536] or
 * 3 width height bytes that do not fit between its offset and n_texel_bytes.  With valid arguments and NULL device
 * pointers it returns DPC_ERR_NULL without touching a device; so it does when face_uv is given without the mat_tex, uv,
 * tex or texels it needs, or face_vn without normals.  Added without a new ABI number.
 * ------------------------------------------------------------------------------------------------- */
size_t dpc_render_meshes_shaded_workspace_bytes(const int32_t* host_meshes, int n_meshes, const int32_t* host_view_mesh,
                                                int views);
int dpc_render_meshes_shaded(const double* verts, int n_verts, const int32_t* faces, const int32_t* face_mat, int n_faces,
                             const double* kd, int n_mats, const double* uv, int n_uv, const int32_t* face_uv,
                             const double* normals, int n_vn, const int32_t* face_vn, const int32_t* mat_tex,
                             const uint8_t* texels, int64_t n_texel_bytes, const int64_t* tex, const int64_t* host_tex,
                             int n_tex, const int32_t* meshes, const int32_t* host_meshes, int n_meshes,
                             const int32_t* view_mesh, const int32_t* host_view_mesh, const double* view_cam, int views,
                             int image_size, int supersample, uint8_t* rgba, uint16_t* depth, int32_t* face_id,
                             int32_t* status, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Opt-in measurement aid (nothing in the reference corresponds to it).  After dpc_profile_enable(capacity)
 * every launch of the fused path is bracketed by hipEvents on its stream; synchronise the stream, then read
 * dpc_profile_count() entries with dpc_profile_get(i, &kernel_name, &milliseconds) and dpc_profile_get_id.  Off by default; the only
 * global state in the library; not usable while a hipGraph is being captured.
 * ------------------------------------------------------------------------------------------------- */
int dpc_profile_enable(int capacity);
int dpc_profile_disable(void);
int dpc_profile_count(void);
int dpc_profile_get(int i, const char** name, float* ms);
/* ABI 14.  The template instantiation entry i launched, as the device symbol's demangled template: "k_gather_hw<64, 8, 3>",
 * "k_zcol_fwdbwd<64, 3, 1>", "k_zcol_fwd_dyn" (no template arguments: the name alone).  Written NUL-terminated into id[cap];
 * DPC_ERR_SHAPE when i is out of range or cap is too small.  What dpc_profile_get names is the kernel family alone. */
int dpc_profile_get_id(int i, char* id, int cap);
/* What an EMPTY begin/end event pair reads on `stream` (synchronising; call outside timed regions): subtract it from
 * dpc_profile_get's figures to compare with rocprofv3's kernel durations. */
int dpc_profile_pair_overhead(void* stream, int pairs, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* DPC_RENDER_H */
