/* libishap_hip.so -- C ABI of the MI355X (gfx950) denoise-and-drag core.
 *
 * The reference (jinli99/iShapEditing) has no native boundary: its hot path is reached through
 * Python calls into stock torch ops.  Each entry point below names the reference function whose
 * arithmetic it replaces (paths relative to the reference root; gd = neural_field_diffusion/
 * guided_diffusion).  Conventions:
 *   - every function returns 0 on success, non-zero on failure; ishap_last_error() gives the
 *     thread-local message; nothing throws across this boundary;
 *   - all tensors are caller-allocated DEVICE buffers (torch owns memory); dims are explicit;
 *   - `stream` is a hipStream_t (0 = default stream); calls only enqueue work, they never sync;
 *   - torch-visible tensors use the reference's layouts (NCHW, fp32 unless noted).
 */
#ifndef ISHAP_H
#define ISHAP_H
#ifdef __cplusplus
extern "C" {
#endif

const char* ishap_last_error(void);
/* Asynchronous device-side failures (the reference's analogue: a CUDA error raised by a later torch call).  A kernel of
 * this library that cannot go on correctly -- today: a bounded cross-workgroup wait that gave up -- poisons its outputs
 * with NaN and raises a process-wide status word; every ishap_unet_* call that enqueues work checks the word first and
 * fails (-3, message in ishap_last_error) if an EARLIER launch raised it.  This call checks on demand, e.g. after a
 * stream synchronise at the end of a loop: 0 = no failure since the last report; the word is cleared once reported. */
int ishap_device_status(void);
/* Tenancy.  The group-local GroupNorm kernels of the small maps run several workgroups per (image, group) that meet INSIDE
 * one launch (gd/nn.py:16-18 needs group-wide sums); such a grid only completes when all of its workgroups are resident
 * together.  Within one process the library arbitrates: per device, ONE (model context, stream) pair at a time may launch
 * such grids; a call on another context / thread / stream that arrives while the holder's work is still in flight runs the
 * same kernels with one workgroup per group, and the 8x8-map AttentionBlock kernel (which also hands data between workgroups
 * inside a launch) as two launches of the same code (BITWISE the same values either way, a few microseconds slower per
 * launch) -- no action needed.
 * The library is otherwise SINGLE-TENANT per GPU: another PROCESS using the same device, or a caller stream created with a
 * compute-unit mask, can keep part of such a grid from becoming resident; the wait is bounded, and the failure is reported
 * as described above (status word, NaN outputs, -3 from the next call), never a hang or a silently wrong result.
 * ishap_rendezvous_would_grant: diagnostic, no side effects -- 1 if a launch sequence of `owner` (a model context, or NULL
 * for the stand-alone operator calls) on `stream` would be allowed in-launch rendezvous right now. */
int ishap_rendezvous_would_grant(const void* owner, void* stream);
int ishap_version(void);   /* 2 since ishap_mesh_smooth takes (and checks) the size of its scratch buffer; 3 since ishap_step_coefs
                            * ends with rng / rng_seed / rng_offset / noise_out; 4 since the batched drag calls (ishap_drag_batch_*,
                            * ishap_ddpm_step_guided_scales); 5 since ishap_igemm_run / ishap_igemm_reduce; 6 since
                            * ishap_triplane_fit_loss_grad / ishap_triplane_reg_*; 7 since
                            * the mesh metrics (ishap_mesh_distance, ishap_hausdorff, ishap_group_field_stats); 8 since
                            * ishap_arap / ishap_arap_scratch_bytes / ishap_nearest_vertices; 9 since ishap_attention_run /
                            * ishap_attention8_run; 10 since ishap_group_norm32_plan replaced ishap_group_norm32_parts; 11 since
                            * the headless renderer (ishap_camera, ishap_render_mesh, ishap_render_scratch_bytes, ishap_unproject);
                            * 12 since the winding numbers (ishap_mesh_winding, ishap_cloud_winding, ishap_cloud_areas,
                            * ishap_winding_scratch_bytes) and sdf == 2 / sdf == -2 of ishap_mesh_distance (sign by winding
                            * number for a counter-clockwise / a clockwise mesh; before 12 both values meant parity); 13 since ishap_group_norm32_run;
                            * 14 since the front end for clouds without normals (ishap_cloud_knn, ishap_cloud_normals,
                            * ishap_cloud_orient, ishap_cloud_orient_scratch_bytes); 15 since the snapshot of a kept forward
                            * (ishap_unet_snapshot_save / _restore / _drop / _bytes); 16 since the connected components of a
                            * volume (ishap_volume_label, ishap_volume_components_*, ishap_volume_flip); 17 since the region
                            * weights of the drag loss (`weights` / `weights_stride` of ishap_drag_batch_args, ishap_region_plane_weights, ishap_region_plane_weights_scratch_bytes);
                            * 18 since the decoder's field in space (ishap_triplane_field_grad, ishap_triplane_project); 19 since
                            * the part edits (ishap_region_select, ishap_region_handles, ishap_region_handles_scratch_bytes,
                            * ishap_region_transform); 20 since ishap_unet_block_grad; 21 since the handle
                            * tracking (ishap_drag_track, ishap_drag_track_scratch_bytes); 22 since the closed-loop drag
                            * (ishap_drag_batch_retarget, ishap_drag_batch_retarget_each); 23 since the exact
                            * distance transform (ishap_edt, ishap_edt_scratch_bytes) and the marks and feathered map of the
                            * regions (ishap_region_plane_marks, ishap_region_plane_feather, ishap_region_plane_feather_scratch_bytes);
                            * 24 since the volume constraints (ishap_constraint_setup, ishap_constraint_setup_scratch_bytes,
                            * ishap_constraint_loss_grad); 25 since the sparse high-resolution surface
                            * (ishap_triplane_decode_bricks, ishap_sparse_*); 26 since the quadric vertex clustering
                            * (ishap_mesh_simplify_scratch_bytes, ishap_mesh_simplify_count, ishap_mesh_simplify_emit); 27 since the
                            * single-edit drag interface was REMOVED (ishap_drag_args, ishap_drag_setup, ishap_drag_loss_grad,
                            * ishap_drag_loss_cotangent, ishap_drag_retarget): one edit is the ishap_drag_batch_* call of the same
                            * name on an ishap_drag_batch_args with E = 1, handle_offsets = {0, B}, cof = {cof} and a scratch of
                            * ishap_drag_batch_scratch_bytes(1, W, ld) bytes */

/* ---------------------------------------------------------------- UNet (gd/unet.py:396-671) */
typedef struct ishap_unet ishap_unet;

typedef struct {
  int image_size;          /* 128 */
  int in_channels;         /* 96 */
  int model_channels;      /* 256 */
  int out_channels;        /* 192 (learn_sigma) */
  int num_res_blocks;      /* 2 */
  int n_mult;              /* length of channel_mult */
  int channel_mult[8];     /* (1,1,2,3,4) for image_size 128, gd/script_util.py:151-161 */
  int n_att;
  int attention_ds[8];     /* downsample rates with attention: image_size // res, script_util.py:163-165 */
  int num_head_channels;   /* 64 */
  int max_batch;           /* largest N a forward may be called with */
} ishap_unet_config;

/* UNetModel.__init__ with use_scale_shift_norm, resblock_updown, use_fp16 (drag_utils.py:44-57):
 * builds the block graph, sizes the activation arena and workspaces on `device`. */
int ishap_unet_create(const ishap_unet_config* cfg, int device, ishap_unet** out);
void ishap_unet_destroy(ishap_unet* u);

/* state_dict key table (same names/shapes torch gives the reference model; drag_utils.py:229-230
 * loads with strict=True).  shape has up to 4 entries. */
int ishap_unet_num_params(const ishap_unet* u);
int ishap_unet_param_info(const ishap_unet* u, int index, char* name, int name_cap, int* ndim, long long* shape);
/* model.load_state_dict + convert_to_fp16 (gd/unet.py:618-624, gd/fp16_util.py:14-21) for one tensor:
 * `data` = fp32 device buffer of `numel` values in the reference's layout.  Conv weights are re-packed
 * to fp16 MFMA operands (forward and input-gradient forms); torso conv biases are rounded through fp16. */
int ishap_unet_load_param(ishap_unet* u, const char* name, const float* data, long long numel, void* stream);
int ishap_unet_params_loaded(const ishap_unet* u);   /* number of distinct tensors loaded so far */

/* UNetModel.forward(x, timesteps, feat_layer) (gd/unet.py:634-671) with timesteps already mapped to the
 * original 0..999 index (gd/respace.py:122-127).
 *   x            [N][in_channels][S][S] fp32
 *   timesteps    HOST array of N floats
 *   feat_layer   output-block index whose activation is tapped (h.clone() at unet.py:665-666), or -1
 *   out          [N][out_channels][S][S] fp32
 *   inter_feat   optional [N][C_tap][S_tap][S_tap] fp16 copy of the tap in the reference layout (may be NULL;
 *                the tap always stays resident inside the context for ishap_drag_* / backward)
 *   keep_for_backward  non-zero: keep every intermediate needed by ishap_unet_backward_input */
int ishap_unet_forward(ishap_unet* u, const float* x, const float* timesteps, int N, int feat_layer,
                       float* out, void* inter_feat, int keep_for_backward, void* stream);
int ishap_unet_tap_shape(const ishap_unet* u, int feat_layer, int* channels, int* size);
/* device pointer of the resident tap of the last forward: NHWC fp16 [N][S_tap*S_tap][C_tap] */
const void* ishap_unet_tap_ptr(const ishap_unet* u);
/* keep_for_backward is a bit set: bit 0 = keep what a following backward re-reads; bit 1 (with feat_layer >= 0) = the part of the
 * network AFTER the tapped output block (the remaining output blocks and the fp32 head) is only PLANNED by the forward and later
 * enqueued on a stream owned by the context.  The drag step needs only the tap for its loss and backward pass
 * (drag_utils.py:355-384), the model output only for the DDPM update after them (:385-393): the two then run side by side.
 * `out` is complete on a stream only after ishap_unet_join_tail(u, that stream); the next ishap_unet_forward, a
 * full-depth backward and ishap_unet_block_output join by themselves.
 * LIFETIME: with bit 1 the library keeps the raw `out` pointer and writes through it when the tail runs -- `out` must stay allocated until ishap_unet_join_tail has been called for this forward (or the next
 * forward / full-depth backward has joined it); freeing it earlier lets the tail write into memory that may have a new owner. */
int ishap_unet_join_tail(ishap_unet* u, void* stream);
/* Enqueues the planned tail on the context's own stream, behind the point the backward pass marked after its first output
 * blocks (or behind the tap when no backward ran).  No-op when nothing is planned; ishap_unet_join_tail runs a plan that was
 * never enqueued.  On failure the launches already enqueued stay ordered before the next join (the context remains usable). */
int ishap_unet_run_tail(ishap_unet* u);
/* Diagnostics (contexts created with ISHAP_BWD_MARKS=1 in the environment; otherwise returns 0): elapsed milliseconds from the start of
 * the last backward pass to the timing event recorded after each of its blocks -- tags: 0 start, 100 + i after output block i, 200
 * after the middle block, 300 + i after input block i, 999 end -- and to the begin / end of the forward tail that ran beside it on the
 * context's side stream (-1 when none did).  Returns the number of marks written (<= cap); synchronises with the device. */
int ishap_unet_marks(ishap_unet* u, int* tags, float* ms, int cap, float* tail_begin_ms, float* tail_end_ms);
/* copy it into a caller buffer of N*S_tap^2*C_tap halfs (the guidance cache of drag_utils.py:275-276, kept
 * on the device in the tap's own layout instead of resized fp32 copies on the host) */
int ishap_unet_copy_tap(const ishap_unet* u, void* dst, void* stream);
/* The output of any TimestepEmbedSequential of the last forward(keep_for_backward=1): group 0 = input_blocks[index]
 * (the `hs` list, gd/unet.py:658-660), 1 = middle_block (:661), 2 = output_blocks[index] (:662-666).  Writes the
 * block's channel count and side to *channels / *size; when dst is non-NULL also copies the activation as fp16
 * [N][channels][size][size] (the reference's layout).  Parity tests use it to localise a mismatch to one block. */
int ishap_unet_block_output(const ishap_unet* u, int group, int index, int* channels, int* size, void* dst_nchw_f16,
                            void* stream);
/* The gradient maps of the last ishap_unet_backward_input / ishap_unet_backward_from_output (ABI 20), block by block: group and
 * index as for ishap_unet_block_output; part 0 = the gradient w.r.t. the block's OUTPUT, summed over all of its consumers (for an
 * input block: the block after it plus its skip connection); parts 1 and 2 (group 2 only) = the gradient w.r.t. the `h` and the
 * `skip` half of an output block's concatenated input (gd/unet.py:663).  Writes the map's channel count and side to *channels /
 * *size; when dst is non-NULL also copies the stored fp16 values, untouched (a loss scale stays in them), as
 * [N][channels][size][size].  The pass keeps no copy: it records where each map was written, and the maps stay there until the
 * next forward, backward or snapshot restore on the context -- a read after one of those fails, as does a read before any
 * backward, of an output block above the one the backward started from, or of parts 1 / 2 outside group 2.  Part 0 of the block a
 * backward from the tap started at IS the caller's cotangent: it is read through the pointer that call was given, which must
 * still be allocated.  Tests use it to pin each block's vector-Jacobian product on its own. */
int ishap_unet_block_grad(const ishap_unet* u, int group, int index, int part, int* channels, int* size, void* dst_nchw_f16,
                          void* stream);
/* Optional, ahead of a sampling loop: compute the timestep-embedding products of n timesteps once (timestep_embedding,
 * time_embed and every ResBlock's emb_layers, gd/unet.py:651,245-250 -- none of them depends on x).  A later
 * ishap_unet_forward whose timesteps all equal one prepared value reuses its row and skips those four launches; any other
 * forward computes them as before.  Results are bit-identical either way.  n = 0 drops the prepared rows; loading a
 * parameter drops them too.  Call it between steps, not between a kept forward and its backward (that forward's
 * intermediates are invalidated if it used a prepared row). */
int ishap_unet_prepare_timesteps(ishap_unet* u, const float* timesteps, int n, void* stream);
/* Device bytes the context holds besides the packed weights: activation arena + split-K partials + GroupNorm scratch
 * (SURVEY 8b's ishap_workspace_bytes; the context allocates them itself at create time, sized by dry runs of
 * forward + backward at every batch size 1..max_batch), plus the snapshot buffers below once one has been saved. */
long long ishap_unet_workspace_bytes(const ishap_unet* u);

/* Snapshot of a kept forward (ABI 15).  A drag edit's first guided step runs the model on the same latent, at the same
 * timestep, through the same weights in every edit of a loaded shape (drag_utils.py:309: img = self.w.clone()), so its
 * forward -- not its loss or backward, which depend on the handles -- can be run once and put back for the later edits.
 * ishap_unet_snapshot_save: valid after ishap_unet_forward with keep_for_backward bit 0; orders `stream` behind a planned
 *   tail (as ishap_unet_join_tail) and copies, on `stream`, what a later ishap_unet_backward_input reads: the activation arena
 *   and the GroupNorm-statistics arena below the forward's marks -- below the planned tail's when the forward planned one, the
 *   backward from the tap reads nothing of the blocks after it -- and the FiLM rows of the forward's timesteps (the snapshot
 *   owns its copy: a later ishap_unet_prepare_timesteps does not touch it), together with the host records that point into
 *   them (saved tensors of every layer, block outputs, the tap).  Buffers are allocated on first use and kept; a second save
 *   replaces the first.
 * ishap_unet_snapshot_restore: orders `stream` behind any pending tail, copies the bytes back to the same offsets and puts the
 *   host records back.  Afterwards ishap_unet_tap_ptr, ishap_unet_copy_tap and ishap_unet_backward_input (any number of
 *   times) behave as after the forward the snapshot was taken of; the model output is the caller's to keep.  When that
 *   forward had planned a tail, the blocks after the tap are not part of the snapshot: ishap_unet_backward_from_output and
 *   ishap_unet_block_output past the tap fail on the restored state.
 * Both return 0, a negative error, or 1 = unavailable while the per-launch profile records (between ishap_profile_begin and
 * ishap_profile_end: a recorded edit runs, and counts, every forward) -- the caller then runs the ordinary forward.  A restore
 * without a valid snapshot is an error and enqueues nothing.  A snapshot stops being valid when a parameter is loaded
 * (ishap_unet_load_param) and when a forward runs with another batch size or another feat_layer than the snapshot's.
 * ishap_unet_snapshot_drop frees the buffers; ishap_unet_snapshot_bytes is their size (0 when there are none). */
int ishap_unet_snapshot_save(ishap_unet* u, void* stream);
int ishap_unet_snapshot_restore(ishap_unet* u, void* stream);
int ishap_unet_snapshot_drop(ishap_unet* u);
long long ishap_unet_snapshot_bytes(const ishap_unet* u);

/* d(sum(tap * cot)) / dx through output block feat_layer ... input block 0: what loss.backward()
 * computes for img.grad at drag_utils.py:383, without the weight gradients the reference discards.
 *   cot_nhwc   fp16 cotangent of the tap in the tap's resident layout [N][S_tap^2][C_tap], already
 *              multiplied by the loss scale *scale2[0] (see ishap_grad_to_scaled_f16)
 *   scale2     device float[2] = {scale, 1/scale} or NULL for scale 1
 *   dx         [N][in_channels][S][S] fp32 = gradient w.r.t. x (loss scale removed) */
int ishap_unet_backward_input(ishap_unet* u, const void* cot_nhwc, const float* scale2, float* dx, void* stream);
/* same, from a cotangent of the model output [N][out_channels][S][S] fp32 (full-depth backward,
 * drag_utils.py:458 in train_triplane) */
int ishap_unet_backward_from_output(ishap_unet* u, const void* cot_out, int cot_is_f16, const float* scale2, float* dx,
                                    void* stream);
/*   cot_out: fp32, or fp16 already multiplied by scale2[0] (ishap_grad_to_scaled_f16); scale2 as above */

/* ---------------------------------------------------------------- GroupNorm32 alone (gd/nn.py:16-18,92-99)
 * normalization(C) = GroupNorm32(32, C): statistics and normalisation in fp32 on x.float(), eps 1e-5, result cast back
 * to the torso's fp16; followed by nn.SiLU in ResBlock.in_layers / out_layers and the head (gd/unet.py:179-183,
 * 205-209, 612-614).  The executor fuses this into the neighbouring kernels and picks one of several statistics
 * routes by map size; these calls run a chosen route on a caller-given tensor, so the reference's own primitive
 * fixtures reach each of them.
 *   x, y, g, dx   NHWC fp16 [N][H*W][C]        stats  [N][32][2] fp32 (mean, rstd): written by the forward, read by the backward
 *   silu          0: y = GN(x);  1: y = SiLU(GN(x))
 *   route         0 = the executor's choice for this map; 1 = two-pass statistics; 2 = group-local, one workgroup per
 *                 (image, group); 3 = group-local, several workgroups meeting in the in-launch rendezvous; 4 (forward
 *                 only) = fixed-point per-channel sums gathered by an implicit-GEMM epilogue (C % 64 == 0)
 *   scratch       device buffer of ishap_group_norm32_scratch_bytes(N, H*W, C) bytes (contents irrelevant) */
long long ishap_group_norm32_scratch_bytes(int N, int HW, int C);
int ishap_group_norm32(const void* x_nhwc_f16, const float* gamma, const float* beta, int N, int H, int W, int C, int silu,
                       int route, void* y_nhwc_f16, float* stats, void* scratch, void* stream);
/* input gradient of sum(y * g) w.r.t. x (no parameter gradients), as autograd derives it at drag_utils.py:383 */
int ishap_group_norm32_backward(const void* g_nhwc_f16, const void* x_nhwc_f16, const float* stats, const float* gamma,
                                const float* beta, int N, int H, int W, int C, int silu, int route, void* dx_nhwc_f16,
                                void* scratch, void* stream);
/* Which launch one GroupNorm pass gets, without running anything and without a GPU (the compute-unit count that bounds `parts` is
 * the current device's, 256 where there is none): a pass over [N][H*W][C] -- forward, or backward != 0 for the input gradient with
 * gmode 0 / 1 / 2 = the upstream gradient at the same / half (the forward pooled) / twice (the forward upsampled) the resolution;
 * pending != 0: the input (backward: the upstream gradient) is still the split-K slices of its producer; film / act / pool: the
 * fused FiLM, SiLU and 2x2 average pool.  route as above, and *route_out = the route taken (route 0 resolved as the executor does,
 * ISHAP_LOCAL_GN included; a backward pass off the small maps takes 1).  Group-local routes (2, 3): parts = workgroups per (image,
 * group) (> 1: the in-launch rendezvous is exercised), vec = channels per lane, the grid is (grid_x, grid_y) workgroups of
 * `threads`, lds_bytes of dynamic LDS, xcd = how the parts are dealt to workgroups (ISHAP_GN_XCD; 0 with one part).  Full-map routes (1, 4): the apply kernel's launch, parts = 0.  kernel: the kernel's name
 * with its template arguments; -2 when kernel_cap is too small.  Outputs may be NULL. */
int ishap_group_norm32_plan(int N, int H, int W, int C, int backward, int pending, int film, int act, int pool, int gmode, int route,
                            int* route_out, int* parts, int* vec, int* threads, int* grid_x, int* grid_y, int* lds_bytes,
                            int* xcd, char* kernel, int kernel_cap);

/* ONE GroupNorm launch as the executor builds it (ABI 13): every option of the forward pass y = act(film(GN(x))) and of its input
 * gradient, on any route, through the functions the UNet executor itself goes through (gn_route, gn_local_fill / gn_local_launch,
 * gn_bwd_local_fill / gn_bwd_local_launch, gn_stats_launch, gn_apply_launch, gn_backward_launch: csrc/norm.h).  Tensors are NHWC
 * fp16 [N][H*W][C] unless said otherwise; pointers that an option does not use stay NULL.
 *   backward      0: forward; 1: input gradient
 *   route         0 = the executor's choice; 1 = full map, two-pass statistics (backward: two-pass sums); 2 / 3 = group-local with
 *                 one / several workgroups per (image, group); 4 (forward) = full map, statistics finalised in the apply kernel from
 *                 per-channel fixed-point sums: the caller's `sums` (`sums2`), or, with sums NULL, those an identity 1x1 convolution
 *                 gathers in its epilogue (C % 64 == 0, N*H*W % 64 == 0, H*W % 64 == 0 at N > 1)
 *   film, act     FiLM `h * (1 + scale) + shift` (needs act) with emb = per image (scale[C] | shift[C]) fp32, emb_ld floats apart; SiLU
 *   scratch       ishap_group_norm32_scratch_bytes(N, H*W, C) bytes
 * forward:
 *   x             the input; with x2: channels [0, csplit) [N][H*W][csplit], x2 the rest [N][H*W][C - csplit], and xcopy receives the
 *                 concatenation [N][H*W][C] (csplit % 8 == 0, % 32 on the group-local routes; on the full map only with sums, sums2)
 *   pool          2x2 mean of the activated map (even H, W; SiLU, no FiLM): out is [N][H/2*W/2][C], xpool (optional) the pooled input
 *   split         the head's form (full map only; SiLU, no FiLM, no pool): out is [N][H*W][3C] = hi | lo | hi
 *   out           the result;  stats_out [N][32][2] (mean, rstd): required on route 1, optional elsewhere
 *   sums, sums2   route 4: [N][channels][2] 64-bit fixed point (sum * 2^24, sum of squares * 2^20) of x (and x2)
 * backward:
 *   g             the gradient arriving at y: same resolution (gmode 0), [N][H/2*W/2][C] each cell's share /4 (gmode 1, even H, W),
 *                 [N][2H*2W][C] the four copies added (gmode 2);  add: optional addend indexed like g;  add2: optional addend
 *                 [N][H*W][C];  x, stats: the forward's input and (mean, rstd)
 *   dx            the result; with csplit != 0 channels [0, csplit) go to dx and the rest to dx2, each dense
 *   sums_ready    route 1: csums [N][C][2] (sum dyh, sum dyh * xhat, both * 2^24) are the caller's; else they are gathered here
 * pending source (group-local routes only): nslab >= 1 fp32 slices [nslab][rows][channels] at ws, zstride floats apart, stand for
 *   the forward's x (channels = csplit with x2, else C; + bias + bias2 + res, res [rows][ldr] fp16, at (H/2, W/2) with res_ups;
 *   x stays NULL and ya receives the fp16 tensor) or for the backward's g (no bias, no residual).
 * launch == 0: check the descriptor and report; no HIP call, works without a GPU.  *route_out = the route taken, *parts_out = the
 * workgroups per (image, group) that ran (0 on a full-map route; 1 on route 3 when the rendezvous tenancy was not granted),
 * kernel = the kernel's name with its template arguments.  A descriptor outside the contract is refused (-2) before any HIP call. */
typedef struct {
  int backward, N, H, W, C, route, film, act;
  int pool, split;                 /* forward */
  int gmode, sums_ready;           /* backward */
  int csplit, emb_ld;
  const float *gamma, *beta, *emb;
  void* scratch;
  const void *x, *x2;
  void *xcopy, *out, *xpool;
  float* stats_out;
  const long long *sums, *sums2;
  const void* g;
  const float* stats;
  const void *add, *add2;
  void *dx, *dx2;
  long long* csums;
  const float* ws;                 /* pending source */
  int nslab, ldr, res_ups, reserved_;
  long long zstride;
  const float *bias, *bias2;
  const void* res;
  void* ya;
} ishap_group_norm_desc;
int ishap_group_norm32_run(const ishap_group_norm_desc* d, int launch, void* stream, int* route_out, int* parts_out, char* kernel,
                           int kernel_cap);

/* ------------------------------------------- diffusion step (gd/gaussian_diffusion.py:232-331, 400-510) */
typedef struct {
  float min_log;        /* posterior_log_variance_clipped[t]  (float64 table cast to fp32, :1035-1048) */
  float max_log;        /* log(betas[t]) */
  float sqrt_recip;     /* sqrt_recip_alphas_cumprod[t] */
  float sqrt_recipm1;   /* sqrt_recipm1_alphas_cumprod[t] */
  float coef1, coef2;   /* posterior_mean_coef1/2[t] */
  float nonzero;        /* 0 when t == 0 else 1 */
  int clip_denoised;
  int mode;             /* 0: mean + sqrt(var)*noise (p_sample_guidance :503/:508)
                           1: mean + exp(0.5*logvar)*noise (p_sample :443)
                           2: mean + variance_noise (:498-499; `noise` holds variance_noise)
                           3: DDIM (ddim_sample :654-705): x0*ddim_a + ddim_b*eps(x0) + nonzero*ddim_sigma*noise */
  float ddim_a;         /* sqrt(alphas_cumprod_prev[t]) */
  float ddim_b;         /* sqrt(1 - alphas_cumprod_prev[t] - sigma^2) */
  float ddim_sigma;     /* eta * sqrt((1-abar_prev)/(1-abar)) * sqrt(1 - abar/abar_prev) */
  /* round 5: the step draws its own noise (the reference's th.randn_like(x), gaussian_diffusion.py:443 / :493) when rng != 0 and
   * `noise` is NULL -- no randn launch and no noise tensor in front of the step.  Philox4x32-10 (Salmon et al., Random123) with
   * key = rng_seed ^ 0x9E3779B97F4A7C15 and counter = {index of the 4-float vector in x (64 bit), rng_offset (64 bit)}; the four
   * words become four standard normals by two Box-Muller pairs (u = ((w >> 8) + 0.5) * 2^-24): element 4 i + j of x takes normal j
   * of vector i.  u is the fp32 number: (float)(w >> 8) + 0.5f needs 25 bits from 2^23 on and rounds to even there, so u lies in
   * (0, 1] and is up to 2^-25 from the exactly formed value -- visible only at u0 -> 1, where the radius sqrt(-2 log u0) goes to
   * 0 (u0 == 1: both normals of the pair are 0).  noise_out: optional [N][C][HW] that receives the noise used (the dict's "noise"). */
  int rng;
  unsigned long long rng_seed, rng_offset;
  float* noise_out;
} ishap_step_coefs;
/* any of sample / pred_xstart / variance / mean may be NULL; noise NULL = zeros (or drawn, ishap_step_coefs::rng); variance_in optional.
 * `variance` receives the LEARNED variance exp(log_variance) also when variance_in is given: variance_in replaces it in the
 * sample's noise term and in `guided` only (the reference's dict returns the caller's own tensor then, :510, which the caller
 * already holds).  `nonzero` multiplies the noise term as given, in modes 0, 1 and 3.  A `noise` that is given wins over
 * `rng`; noise_out is then not written.  clip_denoised is torch's x.clamp(-1, 1): +-inf become +-1, a NaN pred_xstart stays
 * NaN and reaches mean, sample and guided.  Checked launch by launch against float64 in tests/test_gpu_step_oracle.py. */
int ishap_ddpm_step(const float* x, const float* model_out, const float* noise, const float* variance_in,
                    const ishap_step_coefs* k, int N, int C, int HW,
                    float* sample, float* pred_xstart, float* variance, float* mean, void* stream);
/* The step of p_sample_guidance (mode 0) and the guided update of the drag loop in ONE pass (round 5; gd/gaussian_diffusion.py:
 * 446-510 followed by drag_utils.py:384-392): guided = sample + variance * (scale * grad [* *grad_mul_dev]) with the sample and
 * variance this step computes; `sample` / `variance` are optional outputs (null: not written). */
int ishap_ddpm_step_guided(const float* x, const float* model_out, const float* noise, const float* variance_in,
                           const ishap_step_coefs* k, int N, int C, int HW, const float* grad, float scale,
                           const float* grad_mul_dev, float* guided, float* sample, float* variance, void* stream);
/* The same with one guidance scale per image (batched drag edits): guided[n] = sample[n] + variance[n] * (scales[n] * grad[n]
 * [* *grad_mul_dev]); scales = device float[N].  Image n is bitwise what ishap_ddpm_step_guided gives with scale = scales[n]
 * and the same noise.  Drawn noise (k->rng, noise NULL) spans the whole batch: image n takes the Philox vectors of its own
 * place in [N][C][HW], a stream of its own but NOT the one a single-image call with the same seed and offset draws. */
int ishap_ddpm_step_guided_scales(const float* x, const float* model_out, const float* noise, const float* variance_in,
                                  const ishap_step_coefs* k, int N, int C, int HW, const float* grad, const float* scales,
                                  const float* grad_mul_dev, float* guided, float* sample, float* variance, void* stream);
/* img = sample + variance * (scale * grad)   (drag_utils.py:384-392); grad_mul_dev: optional device scalar */
int ishap_guided_update(const float* sample, const float* variance, const float* grad, float scale,
                        const float* grad_mul_dev, long long numel, float* out, void* stream);
/* out = a*x + b*y  (forward-noising chain of ddpm_inversion, gd/gaussian_diffusion.py:520-522) */
int ishap_axpby(const float* x, const float* y, float a, float b, long long numel, float* out, void* stream);

/* ---------------------------------------------------------- drag loss (drag_utils.py:141-159, 309-382) */
/* E drag edits in one call, in the launches of one (loss + gradient: terms, gather, finish; + cotangent: terms, gather, scale);
 * one edit is E = 1.  Per edit: its handles (a CSR range of one packed sources / targets array), cof, rounded-texel bitmap, mask
 * count, loss sums and fixed-point scatter buffer; its tap slice edit + e*W*W*ld and guidance slice orig + e*orig_stride.
 * Shared: W, ld, Cc, chmap, r, voxel, l1, and ONE power-of-two loss scale for the whole batch, picked from max|g| over all edits.
 * An edit's loss and fp32 gradient do NOT depend on the edits beside it, bit for bit: they are what the same edit gives alone,
 * as E = 1, because an edit's workgroups do the same work whatever stands beside them.  Its fp16 cotangent is its E = 1 value
 * times the power of two 2^(k_batch - k_alone) of the two loss scales (bitwise where both are normal fp16 numbers).  The
 * input-gradient backward is linear in the cotangent and removes scale2[1] at its end, so a batched backward needs nothing else. */
typedef struct {
  int E;                /* edits, 1..32 */
  int W;                /* side of the tap feature map (64) */
  int ld;               /* channels of the tap (512) */
  int Cc;               /* channels per plane after resize_feat_align (170) */
  const int* chmap;     /* device int[3*Cc]: (plane, c) -> tap channel (resize_feat_align's mapping) */
  const float* sources; /* device [handle_offsets[E]][3]: the handles of all edits, edit by edit */
  const float* targets; /* device, same layout */
  const int* handle_offsets; /* HOST int[E+1], CSR: edit e owns handles [handle_offsets[e], handle_offsets[e+1]); [0] = 0, each range non-empty */
  int r;                /* lattice radius r1 (12) */
  float voxel;          /* 2 / shape_resolution */
  const float* cof;     /* HOST float[E] */
  int l1;               /* loss_type == 'l1' */
  long long orig_stride;  /* halfs between the guidance features of consecutive edits; 0 = every edit reads the same one */
  void* scratch;          /* device, 16-byte aligned, ishap_drag_batch_scratch_bytes(E, W, ld) bytes; zeroed by the setup call,
                           * left zero by every loss call.  Holds, per edit: the gradient scatter (W*W*ld 64-bit fixed-point sums,
                           * so that repeated edits are bitwise identical: integer atomics commute), two 64-bit fixed-point loss
                           * sums, the mask count, the touched bitmap [3*W*W] (3*W*W % 4 == 0; bit 0 = the reference's
                           * rounded-texel sets, bit 1 = target footprints); and once the inverse of chmap [3*ld] */
  long long scratch_bytes;
  const float* weights;   /* ABI 17, read by the loss calls only.  NULL: no weights.  Else the base of device float[E][3*W*W], each
                           * map indexed [plane][row][col] like the touched bitmap; edit e reads weights + e * weights_stride.  The
                           * mask term of an UNTOUCHED texel t of plane p is multiplied by weights[p][t] (>= 0, finite; 0 frees the
                           * texel, > 1 holds it harder), the count it is divided by stays the count of untouched texels, and the
                           * weight of a touched texel is ignored.  A map of exact ones gives bitwise the results of NULL, so an
                           * edit without regions reads a map of ones.  With cof <= 0 there is no mask term and the map is not
                           * used.  Built from 3-D regions by ishap_region_plane_weights. */
  long long weights_stride; /* floats between the maps of consecutive edits (>= 3*W*W), or 0: one map for every edit */
} ishap_drag_batch_args;
long long ishap_drag_batch_scratch_bytes(int E, int W, int ld);
/* once per batch of edits: each edit's rounded-texel bitmap and complement count (drag_utils.py:322-334); also zeroes the loss
 * sums and the scatter buffer, which every loss call below expects zero on entry and leaves zero on return */
int ishap_drag_batch_setup(const ishap_drag_batch_args* a, void* stream);
/* per step: loss (device float[E]) and d loss / d tap as fp32 NHWC [E][W*W][ld] (drag_utils.py:355-383); edit_nhwc_f16
 * [E][W*W][ld] (the resident tap of a batch-E forward) */
int ishap_drag_batch_loss_grad(const ishap_drag_batch_args* a, const void* edit_nhwc_f16, const void* orig_nhwc_f16,
                               float* grad_nhwc, float* loss, void* stream);
/* the same followed by ishap_grad_to_scaled_f16 (below) on that gradient, as three launches instead of ten: the form the
 * guided step uses (drag_utils.py:355-383 up to loss.backward()).  cot_f16 [E][W*W][ld] with the batch's loss scale; bits: device
 * uint32[1]; scale2: device float[2] */
int ishap_drag_batch_loss_cotangent(const ishap_drag_batch_args* a, const void* edit_nhwc_f16, const void* orig_nhwc_f16,
                                    float* grad_nhwc, float* loss, void* cot_f16, unsigned* bits, float* scale2, void* stream);
/* ---------------------------------------------------------- handle tracking (ABI 21; csrc/track.hip)
 * Where each drag handle went, in the feature space the loss reads: for handle b the candidate offset k in [-R, R]^3 (voxels of
 * the handle lattice, relative to K_in[b]) whose patch of the EDITED tap is nearest, in L1 over the (2 rp + 1)^2 lattice positions
 * and Cc channels of each plane, to the patch of the GUIDANCE tap at the source.  Sampling, plane axes and channel gather are the
 * drag loss's; coordinates are sources[b][axis] + voxel * m with the integer m summed first (source side m = i, candidate side
 * m = K_in + k + i), so K_in + k = 0 reads the source lattice bit for bit.  D(b; k) = D_0(kx, ky) + D_1(ky, kz) + D_2(kx, kz);
 * the winner has the smallest D, then the smallest kx^2 + ky^2 + kz^2, then the lowest ((kz+R) side + ky+R) side + kx+R,
 * side = 2 R + 1.  K_out[b] = K_in[b] + k*, dist[b] = D(k*), dist0[b] = D(0).  No atomics: results are bitwise repeatable and a
 * handle's do not depend on the other handles or edits of the call.  Read-only on both taps.
 *   edit_nhwc_f16 [E][W*W][ld]; orig_nhwc_f16: edit e's guidance at + e * orig_stride halfs (0: one guidance tap for all edits)
 *   chmap device int[3][Cc]; sources device float[Btot][3]; handle_offsets HOST int[E + 1] (CSR, as ishap_drag_batch_args)
 *   K_in, K_out device int[Btot][3] (may be the same buffer); dist, dist0 device float[Btot]
 *   volume: NULL, or device float[Btot][side^3], every D(b; k) at the linear index above
 *   scratch: device, 16-byte aligned, ishap_drag_track_scratch_bytes(E, Btot, R, rp, Cc) bytes
 * 0 <= R <= 8, 0 <= rp <= 4, 1 <= E <= 32, every edit at least one handle: anything else is an error before any launch (the
 * scratch size call returns -1).  Two launches. */
long long ishap_drag_track_scratch_bytes(int E, int Btot, int R, int rp, int Cc);
int ishap_drag_track(const void* edit_nhwc_f16, const void* orig_nhwc_f16, long long orig_stride, int W, int ld, int Cc,
                     const int* chmap, const float* sources, const int* handle_offsets, int E, float voxel, int R, int rp,
                     const int* K_in, int* K_out, float* dist, float* dist0, float* volume, void* scratch, long long scratch_bytes,
                     void* stream);
/* ---------------------------------------------------------- closed-loop drag (ABI 22; csrc/retarget.hip)
 * Re-aim the drag loss at the tracked handles, once per tracked step.  For handle b of edit e, with K[b] its tracked integer voxel
 * offset from the source (ishap_drag_track's K_out; zeros before the first step), in double with contraction off, order x, y, z:
 *   T = (final_target - source) / voxel,  rem = T - K,  d = |rem|
 *   goal = final_target (a bit copy)                               if d <= step
 *        = (float)(source + voxel * (K + step * rem / d))          otherwise
 *   remaining[b] = (float)d,  arrived[b] = d <= arrive,  done[e] = every handle of edit e has arrived
 * and the call rebuilds what ishap_drag_batch_setup derives from its targets as if it had been given targets = goals: `touched`
 * (both bits) and the mask counts.  The fixed-point scatter buffer, the loss sums (every loss call leaves both zero) and
 * chan_weight (independent of the handles) are not touched, so a loss call may follow at once.  With step = +inf the goals are the
 * final targets bit for bit.
 *   a: the struct of the drag calls on the buffers ishap_drag_batch_setup prepared; a->targets is the GOALS buffer, device
 *      float[Btot][3], WRITTEN by this call and read by the loss calls that follow; it must not be final_targets
 *   final_targets device float[Btot][3]; K device int[Btot][3]; step > 0 (may be +inf), arrive >= 0, in voxels
 *   remaining device float[Btot]; arrived device int[Btot]; done device int[E]
 * One launch of E workgroups, 3*W*W bytes of LDS each, no atomics on global memory and no memset: results are bitwise repeatable
 * and an edit's do not depend on the edits beside it.  A null pointer, a step that is not > 0, an arrive that is not >= 0 (NaN
 * fails both), 3*W*W > 65536 and everything the drag calls require are errors before any launch. */
int ishap_drag_batch_retarget(const ishap_drag_batch_args* a, const float* final_targets, const int* K, float step, float arrive,
                              float* remaining, int* arrived, int* done, void* stream);
/* the same with one lead and one arrival radius per edit: steps, arrives HOST float[E] */
int ishap_drag_batch_retarget_each(const ishap_drag_batch_args* a, const float* final_targets, const int* K, const float* steps,
                                   const float* arrives, float* remaining, int* arrived, int* done, void* stream);
/* ---------------------------------------------------------- region-constrained edits (ABI 17; csrc/regions.hip)
 * The weight map of the drag loss's mask term from 3-D regions in the coordinates handles use, [-1, 1]^3.  A region is a union
 * of primitives and one voxel grid; `keep` must not move, `free` may.  Its SHADOW on plane p (axes as the drag loss: plane 0
 * col = x, row = y; plane 1 col = y, row = z; plane 2 col = x, row = z) is a set of plane texels:
 *   box     the texel centre (u = 2 col / (W - 1) - 1, v likewise, in double) lies in the projected rectangle, bounds inclusive;
 *   sphere  (u - cu)^2 + (v - cv)^2 <= r^2 in double;
 *   voxels  uint8 [D][D][D], non-zero = set, indexed [ix][iy][iz] on linspace(-1, 1, D) like a decoded volume, D >= W: every set
 *           voxel marks the texel nearest to it on each plane, t = (2 i (W - 1) + (D - 1)) / (2 (D - 1)) in integers.
 * Every shadow is grown by a Chebyshev radius of `dilate` texels, clipped at the map.  Then weights_out[p][row][col] =
 * keep_weight in the keep shadow, else free_weight in the free shadow, else 1 (keep overrides free).
 * The inherent limit: a plane texel stands for a whole column through the shape, so a region constrains its three shadows, not
 * only its own volume.
 * prims: device array of n_prims entries (NULL when n_prims = 0); keep_voxels / free_voxels: device, either may be NULL (then D
 * is not used); shadow_counts: device int[2] or NULL, receives the texel counts of the keep and the free shadow over the three
 * planes BEFORE dilation (0: the region is thinner than the texel pitch or outside the cube); scratch: device, 16-byte aligned,
 * ishap_region_plane_weights_scratch_bytes(W) bytes, needs no initialisation.  Returns an error code (and launches nothing) for
 * W < 2 or > 4096, D < W or > 4096 with a grid, dilate < 0, non-finite or negative weights, a NULL output. */
typedef struct {
  int kind;        /* 0 box, 1 sphere */
  int role;        /* 0 keep, 1 free */
  double a[3];     /* box: lo; sphere: centre */
  double b[3];     /* box: hi; sphere: b[0] = radius */
} ishap_region_prim;
long long ishap_region_plane_weights_scratch_bytes(int W);
int ishap_region_plane_weights(const ishap_region_prim* prims, int n_prims, const unsigned char* keep_voxels,
                               const unsigned char* free_voxels, int D, int W, int dilate, float keep_weight, float free_weight,
                               float* weights_out, int* shadow_counts, void* scratch, long long scratch_bytes, void* stream);
/* The marks themselves (ABI 23): the inputs of ishap_region_plane_weights without the two weights, the same scratch.
 * marks_out: device uint8 [3][W][W], bit 0 = in the keep shadow, bit 1 = in the free shadow, both after `dilate`. */
int ishap_region_plane_marks(const ishap_region_prim* prims, int n_prims, const unsigned char* keep_voxels,
                             const unsigned char* free_voxels, int D, int W, int dilate, unsigned char* marks_out, int* shadow_counts,
                             void* scratch, long long scratch_bytes, void* stream);
/* The feathered map (ABI 23): the weights ramp over `falloff` texels outside each dilated shadow instead of jumping.  With dk, df
 * the squared texel distances of a texel to the keep and the free shadow of its plane (ishap_edt on the marks, axes = 6; an empty
 * shadow gives ISHAP_EDT_INF) and A[d2] = table[d2] for d2 < table_len, else 0:
 *   a_k = A[dk], a_f = A[df]
 *   w = keep_weight                                          if a_k == 1
 *       free_weight                                          if a_k == 0 and a_f == 1
 *       1                                                    if a_k == 0 and a_f == 0
 *       (1 + (kw - 1) a_k) + ((fw - 1) a_f) (1 - a_k)        otherwise: in double, no contraction, rounded once to float
 * table: DEVICE double[table_len], built on the host as max(0, 1 - sqrt(d2) / falloff) for d2 < ceil(falloff^2), 0 < falloff <= 64
 * texels (1 <= table_len <= 4096): the device takes no square root, so the map is bitwise what the formula gives in double.  A
 * table of one entry (falloff <= 1) is the hard map.  2 <= W <= 1024; scratch: ishap_region_plane_feather_scratch_bytes(W) bytes,
 * 16-byte aligned, no initialisation; everything else as ishap_region_plane_weights.  A feathered region still constrains its
 * three shadows, not only its own volume. */
long long ishap_region_plane_feather_scratch_bytes(int W);
int ishap_region_plane_feather(const ishap_region_prim* prims, int n_prims, const unsigned char* keep_voxels,
                               const unsigned char* free_voxels, int D, int W, int dilate, float keep_weight, float free_weight,
                               const double* table, int table_len, float* weights_out, int* shadow_counts, void* scratch,
                               long long scratch_bytes, void* stream);

/* ---------------------------------------------------------- exact distance transform (ABI 23; csrc/edt.hip)
 * The exact squared Euclidean distance transform of a byte grid, on the caller's stream: no host synchronisation, no allocation.
 *   Grids   seeds: device uint8 [n0][n1][n2], n2 fastest -- the layout of volumes, x slowest.  A voxel is a seed where its byte is
 *           non-zero or, with invert = 1, where it is zero.
 *   Axes    axes is a bit mask: bit a set means distance is measured along axis a.  An axis that is not set is a batch axis:
 *           slices along it never see each other.  axes = 7 is the 3-D transform of a volume; axes = 6 on [3][W][W] is three
 *           independent 2-D transforms of the plane maps.  axes = 0 is an error.
 *   Output  dist2[v] = min over the seeds s of v's slice of sum over the measured axes a of (v_a - s_a)^2, an exact int32;
 *           ISHAP_EDT_INF wherever the slice holds no seed.
 *   Limits  every measured axis is at most 1024 long, so every real distance is below 2^22, far from ISHAP_EDT_INF;
 *           n0 n1 n2 < 2^31; seeds and dist2 do not alias.
 *   Errors  bad sizes, axes outside 1..7, invert outside 0..1, a NULL pointer, aliasing buffers or a scratch smaller than
 *           ishap_edt_scratch_bytes (which is -1 for bad sizes) return an error code and launch nothing.
 * Integer arithmetic only and no atomics: two runs give the same bits.  scratch: device, 4-byte aligned, no initialisation. */
#define ISHAP_EDT_INF (1 << 30)
long long ishap_edt_scratch_bytes(int n0, int n1, int n2, int axes);
int ishap_edt(const unsigned char* seeds, int n0, int n1, int n2, int axes, int invert, int* dist2, void* scratch,
              long long scratch_bytes, void* stream);

/* ---------------------------------------------------------- part edits (ABI 19; csrc/parts.hip)
 * From a region and a rigid motion to handles, targets and free regions, without a voxel going through the host.  Grids are
 * uint8 [D][D][D], non-zero = set, indexed [ix][iy][iz] (x slowest) on linspace(-1, 1, D) like a decoded volume, 2 <= D <= 1024;
 * a voxel's centre is x_i = 2 i / (D - 1) - 1 per axis, in double.  All arithmetic is integer or double, written so that it
 * rounds operation by operation; the only atomics are integer ones, so every result repeats bit for bit.  Each call returns an
 * error code and launches nothing for a size outside its limits, a NULL argument or a non-finite number.
 *
 * ishap_region_select: mask_out[v] = 1 where volume[v] - level > 0 (float, the inside rule of the surface) AND the voxel's centre
 *   lies in the union of the primitives (`role` is ignored; box: lo <= x <= hi on all three axes, bounds inclusive; sphere:
 *   (dx dx + dy dy) + dz dz <= r r) or the voxel is set in `grid` (device, may be NULL); else 0.  prims: device array (NULL when
 *   n_prims = 0).  count: device int[1], the number of set voxels.
 *
 * ishap_region_handles: n farthest-point picks among the set voxels of `mask` (the candidates, M of them).  Pick 0: with
 *   `start` (HOST int[3], a voxel of the grid, set or not) the candidate nearest to it; with start = NULL the candidate farthest
 *   from the centre of the candidates' bounding box, comparing |2 v - (lo + hi)|^2.  Pick r >= 1: the candidate with the largest
 *   squared distance (exact int32) to the picks made so far.  Every tie goes to the lowest linear index (ix D + iy) D + iz.
 *   picks_out: device int[n][3]; dist2_out: device unsigned[n], the squared distance at the time of each pick (pick 0: 0), so
 *   dist2_out[n - 1] is the smallest pairwise squared distance among the picks; M_out: device int[1].  Rounds beyond M write
 *   (-1, -1, -1) and 0.  1 <= n <= 4096.  The rounds are stream-ordered launches that read M and the previous pick from device
 *   memory: no host synchronisation.  scratch: device, 16-byte aligned, ishap_region_handles_scratch_bytes(D, n) bytes (room for
 *   every voxel as a candidate: 8 D^3 bytes and a little), needs no initialisation.
 *
 * ishap_region_transform: the region moved by x -> R (x - pivot) + pivot + t, as an inverse map (no holes).  rigid15: HOST
 *   double[15] = R row-major, pivot, t.  For every destination voxel j: d = x_j - pivot - t; y_a = ((R[0][a] d_0 + R[1][a] d_1) +
 *   R[2][a] d_2) + pivot_a; i_a = rint((y_a + 1) (D - 1) / 2), half to even; mask_out[j] = 1 where every i_a is in [0, D - 1]
 *   and mask[i] is set.  mask_out must not be mask.  count: device int[1], the number of set voxels. */
int ishap_region_select(const float* volume, int D, float level, const ishap_region_prim* prims, int n_prims,
                        const unsigned char* grid, unsigned char* mask_out, int* count, void* stream);
long long ishap_region_handles_scratch_bytes(int D, int n);
int ishap_region_handles(const unsigned char* mask, int D, int n, const int* start, int* picks_out, unsigned* dist2_out, int* M_out,
                         void* scratch, long long scratch_bytes, void* stream);
int ishap_region_transform(const unsigned char* mask, int D, const double* rigid15, unsigned char* mask_out, int* count, void* stream);

/* fp32 gradient -> fp16 cotangent times a power-of-two loss scale picked from max|g| on the device;
 * bits: device scratch uint32[1]; scale2: device float[2] = {scale, 1/scale} */
int ishap_grad_to_scaled_f16(const float* grad, void* out_f16, unsigned* bits, float* scale2, long long numel,
                             void* stream);

/* ------------------------------------- decoder (triplane_decoder/axisnetworks.py:517-562, visualize.py:76-97) */
typedef struct {
  const float* B;       /* net.0._B      [32][64] */
  const float* W1;      /* net.1.weight  [128][128] */
  const float* b1;
  const float* W2;      /* net.3.weight  [128][128] */
  const float* b2;
  const float* w3;      /* net.5.weight  [1][128] */
  const float* b3;      /* net.5.bias    [1] */
} ishap_decoder_weights;
/* (latent * range + middle).reshape(3,32,S,S) (drag_utils.py:295) into channels-last planes [3][S][S][32];
 * range/middle: device float[96] or NULL for 1/0 */
int ishap_planes_prepare(const float* latent, const float* range, const float* middle, int S, float* planes,
                         void* stream);
/* MultiTriplane.forward: logits for explicit coords [npts][3] */
int ishap_triplane_decode_points(const float* planes, int S, const ishap_decoder_weights* w, const float* coords,
                                 long long npts, float* logits, void* stream);
/* create_obj_o3d's dense grid (visualize.py:79-97): axis = device float[res] (torch.linspace(-1,1,res)),
 * volume[res][res][res] with x slowest, no host round trips */
int ishap_triplane_decode_grid(const float* planes, int S, const ishap_decoder_weights* w, const float* axis, int res,
                               float* volume, void* stream);

/* The field in space, extending MultiTriplane.forward (axisnetworks.py:537-562): logits [npts] and grad [npts][3] =
 * d logit / d coordinate at coords [npts][3].  Analytic (bilinear slopes, the sin / cos features, the two ReLU layers); on a
 * cell boundary of a plane floor() decides the cell, so the derivative is the right-sided one.  Points outside every plane
 * have gradient exactly 0.  Requires S >= 2, npts >= 1.  No atomics: bitwise repeatable. */
int ishap_triplane_field_grad(const float* planes, int S, const ishap_decoder_weights* w, const float* coords,
                              long long npts, float* logits, float* grad, void* stream);
/* Project coords [npts][3] onto the zero level set of the same field (axisnetworks.py:537-562).  Per point x = x0,
 * (z, g) = field(x), scale = 1; `iterations` (0..64) times: stop updating once |z| <= tol or |g|^2 < gmin, else try
 * d = -scale z g / max(|g|^2, gmin) with |d| clipped to step_max and x + d clipped into the ball of radius max_move around
 * x0; take the trial (and reset scale to 1) if it lowers |z|, else halve scale.  So |z_out| <= |z at x0| exactly, and
 * |x_out - x0| <= max_move (1 + 4 * 2^-24) for every point (the ball is tested on the rounded fp32 positions).  x_out [npts][3], z_out [npts] (the logit at x_out), normal_out [npts][3] =
 * -g / |g| at x_out: the direction of DECREASING logit, which points outward because logits are positive inside; exactly 0
 * where |g|^2 < gmin.  accepted_out [npts] int32: steps taken.  iterations = 0: logit and normal at the given points.
 * step_max > 0, gmin > 0, max_move >= 0, tol >= 0 (coordinate units).  Bitwise repeatable. */
int ishap_triplane_project(const float* planes, int S, const ishap_decoder_weights* w, const float* coords, long long npts,
                           int iterations, float step_max, float max_move, float tol, float gmin, float* x_out,
                           float* z_out, float* normal_out, int* accepted_out, void* stream);

/* real-shape guidance (drag_utils.py:447-463): prediction = decoder(0, coord); loss = -BCEWithLogitsLoss()(prediction, gt);
 * loss.backward() -- forward and backward of the decoder on sampled points.  W1T / W2T: transposed copies of
 * net.1.weight / net.3.weight.  Outputs: loss[1], dplanes [3][S][S][32] = d loss / d planes, optional logits[npts]. */
int ishap_triplane_points_loss_grad(const float* planes, int S, const ishap_decoder_weights* w, const float* W1T,
                                    const float* W2T, const float* coords, const float* gt, long long npts,
                                    float* dplanes, float* loss, float* logits, void* stream);

/* Volume constraints of a drag edit (csrc/constrain.hip): the same loss at FIXED points with a weight per point,
 *   L = -(1 / wsum) sum_j w_j BCEWithLogits(decoder(planes)(q_j), g_j),
 * and d L / d planes without float atomics: the scatter of the points' bilinear taps is built once as a gather list and
 * summed in a fixed order at every step.  All calls run on `stream`, allocate nothing, do not synchronise with the host,
 * and on bad sizes (1 <= M <= 2^20, 2 <= S <= 1024) or a NULL argument return an error code and launch nothing;
 * ishap_constraint_setup_scratch_bytes is -1 for bad sizes.
 * ishap_constraint_setup, once per edit: coords [M][3] (device) -> row_start int[3 S S + 1], entry int[<= 12 M], entry_w
 * float[<= 12 M].  The 12 taps of every point (three planes x the four taps of the decoder's bilinear cell, out-of-range
 * taps dropped) grouped by texel row (p S + y) S + x: row r owns entries row_start[r] .. row_start[r + 1] - 1,
 * row_start[3 S S] is their number; entry = 4 j + q (point j, tap q: nw ne sw se), ascending within a row; entry_w = the
 * tap's bilinear weight.  The three arrays depend on coords and S alone (integer atomics count, a ranking pass orders):
 * identical from run to run.  The ranking costs (entries of a row)^2 / 64 steps per row.
 * ishap_constraint_loss_grad, once per step, two launches: targets [M] in {0, 1}, weights [M] >= 0, wsum = their sum
 * (> 0; summed in double by the caller), the gather list of the same coords and S; scratch dfeat float[M][32] and
 * partials float[ceil(M / 32)].  Outputs: dplanes [3][S][S][32] with EVERY texel written (0.0 where no tap reaches: no
 * memset is needed), loss[1], optional logits[M] -- the bits ishap_triplane_field_grad returns for the same planes,
 * weights and coords.  A point of weight 0 contributes exactly 0.  Bitwise repeatable.  As with every region feature the
 * constraint acts through the planes; unlike the plane weights of the drag loss it is stated at points of the volume. */
long long ishap_constraint_setup_scratch_bytes(long long M, int S);
int ishap_constraint_setup(const float* coords, long long M, int S, int* row_start, int* entry, float* entry_w,
                           void* scratch, long long scratch_bytes, void* stream);
int ishap_constraint_loss_grad(const float* planes, int S, const ishap_decoder_weights* w, const float* coords,
                               const float* targets, const float* weights, long long M, double wsum, const int* row_start,
                               const int* entry, const float* entry_w, float* dfeat, float* partials, float* dplanes,
                               float* loss, float* logits, void* stream);
/* direct triplane fitting (drag_utils.py:473-550, train_triplane_opt), one Adam step = these two calls:
 * (1) dplanes [3][S][S][32] += d(BCE + pair_w * mse)/d planes and loss_parts[2] += {BCEWithLogits mean, mse} for the batch
 *     coords[idx[i]] / gt[idx[i]] (i < nbatch; coords [P][3], gt [P], idx int32) and the random pairs r = rand_coords[j],
 *     r + 0.01 * rand_noise[j] (j < nrand; [nrand][3] each; points outside [-1,1] sample zeros).  Float atomics: the
 *     low bits of dplanes vary from run to run. */
int ishap_triplane_fit_loss_grad(const float* planes, int S, const ishap_decoder_weights* w, const float* coords,
                                 const float* gt, const int* idx, long long nbatch, const float* rand_coords,
                                 const float* rand_noise, long long nrand, float pair_w, float* dplanes, float* loss_parts,
                                 void* stream);
/* (2) reg_parts[2] = {l2reg, tvreg} of `planes` (axisnetworks.py:564-575, one object), then torch's Adam step (no weight
 *     decay) on grad = dplanes + l2_w * d l2reg + tv_w * d tvreg into planes_out (must not alias planes); m, v: Adam state
 *     [3][S][S][32]; step: device int32 step count, incremented by the call; dplanes is left zeroed.  reg_parts may be NULL.
 *     ws: device double[ISHAP_TRIPLANE_REG_WS].  Bitwise repeatable. */
#define ISHAP_TRIPLANE_REG_WS 576
int ishap_triplane_reg_adam_step(const float* planes, float* planes_out, float* m, float* v, float* dplanes, int S, int* step,
                                 double lr, double beta1, double beta2, double eps, float l2_w, float tv_w, double* ws,
                                 float* reg_parts, void* stream);
/* reg_parts[2] = {l2reg, tvreg} of planes alone (MultiTriplane.l2reg / tvreg); ws as above */
int ishap_triplane_reg_values(const float* planes, int S, double* ws, float* reg_parts, void* stream);
/* chain rule from planes = clamp(sqrt_recip*x - sqrt_recipm1*eps, -1, 1)*range + middle back to the step's inputs
 * (drag_utils.py:448-450, gd/gaussian_diffusion.py:333-338,299-301): g_direct [96][S][S] = explicit d/dx term,
 * cot_out [192][S][S] = cotangent of the model output (eps half; variance half zero) for the UNet backward */
int ishap_x0_grad_to_cotangent(const float* dplanes, const float* range, const float* x, const float* model_out,
                               float sqrt_recip, float sqrt_recipm1, int clip_denoised, int S, float* g_direct,
                               float* cot_out, void* stream);

/* ------------------------------------------------------------------ surface of the decoded volume
 * Replaces the third-party CPU calls after the decode: mcubes.marching_cubes(volume, 0) (visualize.py:100),
 * mesh.filter_smooth_simple(10) (drag_utils.py:300) and the nearest-neighbour part of meshProcess.py:18-35.
 * `method` 1 = MARCHING CUBES (what the reference calls): one vertex per sign-changing grid edge at the linear zero crossing,
 * shared by the cells around the edge (so the vertex count is the marching-cubes vertex count), triangles from a 256-case
 * table derived by tools/make_mc_table.py (PyMCubes' own table is not available here: triangle-level parity unpinned).
 * `method` 0 = marching tetrahedra (6 per cell; extra vertices on face / body diagonals).  Grid coordinates,
 * deterministic voxel order.  volume: device float[res^3], x slowest.
 * Two calls because the caller allocates the outputs: count -> read counts -> emit. */
long long ishap_surface_scratch_bytes(int res);
/* counts: device unsigned[2] = {vertices, triangles} */
int ishap_surface_count(const float* volume, int res, float level, int method, void* scratch, unsigned* counts, void* stream);
/* verts: device float[3*vertices]; tris: device int[3*triangles]; same volume / level / method / scratch as the count call */
int ishap_surface_emit(const float* volume, int res, float level, int method, void* scratch, float* verts, int* tris,
                       void* stream);

/* ------------------------------------------------------------------ sparse high-resolution surface (csrc/sparse_surface.hip)
 * The marching-cubes surface (`method` 1 above: same tables, same tie rule value - level > 0 = inside, same edge interpolation,
 * compiled from one header) of the decoder's field on a FINE grid without its dense volume.
 * Fine grid: R nodes per axis at axis[R] = torch.linspace(-1, 1, R), 9 <= R <= 2048.  Brick: 8^3 cells; nb = ceil((R - 1) / 8)
 * per axis, id = (bx nb + by) nb + bz.  Brick b samples the 9^3 nodes 8 b .. 8 b + 8 per axis, indices above R - 1 clamped to
 * R - 1 (duplicates of the last node: they are never cut).  It owns the nodes and cells of local index 0..7 that exist, the
 * last brick of an axis also node plane 8 when that is the grid's last (R - 1 = 8 nb), and the +x / +y / +z edges leaving its
 * nodes.  Vertices are in fine-grid coordinates.
 * State, all caller-allocated device memory: map unsigned char[nb^3] (0 inactive, 1 seeded, 2 grown), slot_map int[nb^3]
 * (brick -> slot, -1 inactive), list int[<= nb^3] (slot -> brick, discovery order), values float[n][9][9][9] by slot,
 * reach: ishap_sparse_reach_bytes(n) bytes by slot, ZEROED for a brick when it joins (a byte per sample node, bit a = the edge
 * leaving the node along axis a carries a vertex of the result).
 * Every call runs on `stream`, allocates nothing, does not synchronise with the host, and on bad sizes or a NULL argument
 * returns an error code and launches nothing (the *_bytes queries return -1).  Integer atomics only: bitwise repeatable.
 *
 * ishap_sparse_seed_volume: every cell of the coarse dense volume coarse[Rc^3] (x slowest; 2 <= Rc <= 2048) whose 8 corners
 *   are not all on one side of `level` stores 1 into the map bytes of the bricks that overlap the cell's extent, per axis the
 *   bricks ishap_sparse_seed_range gives (a host function, the same integer arithmetic on j (R - 1) against b (Rc - 1): brick b
 *   meets coarse cell j when 8 b (Rc - 1) <= (j + 1)(R - 1) and min(8 b + 8, R - 1)(Rc - 1) >= j (R - 1)).  The map is the
 *   caller's to clear; any other seed source (every brick, an explicit list) is a map the caller fills with 1.  One thread
 *   stores the brick box of its coarse cell, so the grids are bounded against each other: R - 1 <= 64 (Rc - 1) (at most 10^3
 *   bricks a cell), an error otherwise.
 * ishap_sparse_compact: the marked bricks as an ASCENDING list of ids and count[1] = their number (entries beyond
 *   list_capacity are dropped, the count is not).  mode 0: all marked bricks, slot_map = rank or -1 (every entry written);
 *   mode 1: the marked bricks that have no slot yet, slot_map = first_slot + rank; mode 2: all marked bricks, slot_map untouched
 *   (the order of emission).  scratch: ishap_sparse_compact_scratch_bytes(R), 16-byte aligned.
 * ishap_triplane_decode_bricks: values[i][9][9][9] (i < nbricks <= 2^21) of bricks[i] -- a separate instantiation of the dense decode's
 *   tile loop whose coordinates are axis[clamped node index]; no coordinate buffer.  Each logit has the bits
 *   ishap_triplane_decode_grid(axis, R) gives the same node.
 * ishap_sparse_grow, one round over the n active bricks list[0 .. n): floods `reach` through the triangles of every brick's
 *   owned cells (the three edges of a triangle are reached together; a seeded brick reaches every edge its cells cut), records
 *   each newly reached edge with the brick that owns it, marks (map = 2) the inactive bricks among those of the up-to-4 cells
 *   around it (cells outside the grid do not exist) and adds the number of newly recorded edge bits to changed[1].  The caller
 *   compacts (mode 1), decodes and appends the new bricks and repeats until a round leaves changed == 0 and adds no brick.
 *   Then the owner brick of every reached edge is active, and the reached edges are exactly the vertices of the connected
 *   components (triangles joined through shared vertices) of the dense-at-R surface that cut a cell of a seeded brick.
 *   The reached set and the active bricks are that least fixed point whatever the order of the workgroups; the NUMBER of rounds
 *   is not: a brick reads its neighbours' bytes with plain loads while the same launch ors into them, so it may see a new bit
 *   in this round or the next.  Host read-backs of a whole extraction: the seed count after the first compaction (coarse seeds:
 *   the first decode has to be sized), {changed, new bricks} once per round, the counts before emit.
 * ishap_sparse_surface_count / _emit: `ordered` = the active bricks ascending (compact mode 2).  count: counts[2] =
 *   {vertices, triangles}; emit: verts float[3 vertices] over (brick ascending, owned node x-slowest, axis x, y, z), tris
 *   int[3 triangles] over (brick, owned cell x-slowest), neighbour vertices through slot_map -> per-brick vertex offsets.
 *   scratch: ishap_sparse_surface_scratch_bytes(R, n), 16-byte aligned, the same buffer for both calls. */
int ishap_sparse_bricks_per_axis(int R);       /* nb, -1 for R outside 9 .. 2048 */
int ishap_sparse_seed_range(int Rc, int R, int j, int* first, int* last);
int ishap_sparse_seed_volume(const float* coarse, int Rc, float level, int R, unsigned char* map, void* stream);
long long ishap_sparse_compact_scratch_bytes(int R);
int ishap_sparse_compact(const unsigned char* map, int R, int mode, int first_slot, int* slot_map, int* list,
                         long long list_capacity, unsigned* count, void* scratch, long long scratch_bytes, void* stream);
int ishap_triplane_decode_bricks(const float* planes, int S, const ishap_decoder_weights* w, const float* axis, int res,
                                 const int* bricks, long long nbricks, float* values, void* stream);
long long ishap_sparse_reach_bytes(long long nbricks);
int ishap_sparse_grow(const float* values, const int* list, long long nbricks, int R, float level, unsigned char* map,
                      const int* slot_map, unsigned* reach, unsigned* changed, void* stream);
long long ishap_sparse_surface_scratch_bytes(int R, long long nbricks);
int ishap_sparse_surface_count(const float* values, const int* ordered, long long nbricks, int R, float level,
                               const int* slot_map, unsigned* reach, void* scratch, long long scratch_bytes, unsigned* counts,
                               void* stream);
int ishap_sparse_surface_emit(const float* values, const int* ordered, long long nbricks, int R, float level,
                              const int* slot_map, unsigned* reach, void* scratch, long long scratch_bytes, float* verts,
                              int* tris, void* stream);

/* ---------------------------------------------------------------- Mesh simplification (ABI 26, csrc/simplify.hip)
 * Quadric vertex clustering: Open3D's simplify_vertex_clustering(voxel_size, contraction = Quadric | Average) on the device,
 * one pass, integer atomics only, bitwise repeatable and independent of the order of the input.  The reference has no
 * counterpart (its meshes stop at 256^3).  THE RULE (tests/simplify_ref.py restates it in float64 numpy; every float64
 * expression below is evaluated as written, left to right, without fused multiply-add):
 * Inputs: verts float[V][3], tris int[F][3] (device); a grid: origin lo[3] (double), cell size h > 0 (double), dims
 *   g = (gx, gy, gz) >= 1 with gx gy gz <= 2^30.  A triangle with a corner outside 0 .. V - 1 takes part in nothing.
 * Cells: per axis q = ((double)v - lo) / h, c = clamp(floor(q), 0, g - 1) with a NaN floor taken as 0; cell id
 *   (cx gy + cy) gz + cz; local coordinate p = clamp(q - (c + 0.5), -0.5, 0.5), a NaN p taken as 0.
 * Clusters: the non-empty cells, numbered in ascending cell id.
 * Per-cluster sums, all 64-bit integers (one row of 16 per cluster): [0] vertex count; [1..3] sum rint(p 2^32) per axis;
 *   [4] lowest vertex index; [5..14] the quadric; [15] sum ceil(w).  Every triangle whose corners are valid adds, once per corner,
 *   to the cluster of that corner in that corner's cell frame: P = q (unclamped), N = (P1 - P0) x (P2 - P0),
 *   L = sqrt((Nx Nx + Ny Ny) + Nz Nz); skipped if L is 0 or not finite; n = N / L, w = L / 2,
 *   d = -((nx px + ny py) + nz pz) with the corner's p; the ten values w (a b) over (a, b) = nx nx, nx ny, nx nz, ny ny, ny nz,
 *   nz nz, nx d, ny d, nz d, d d, each added as rint(value 2^36); and ceil(w) to [15].  A triangle with w >= 2^26 adds 2^26 to
 *   [15] and no quadric entry.
 * Overflow guard: |n| <= 1 and |d| <= sqrt(3) / 2 bound every quadric entry by sum w, so below sum ceil(w) = 2^26 no sum
 *   reaches 2^62.  If the [15] of a cluster that a kept triangle references reaches 2^26 (contraction quadric), count sets
 *   bit 0 of its status word: the caller must not emit (use a larger cell, or contraction average).  Nothing wraps silently.
 * Representative of a cluster, x in cell units: count 1: the vertex itself, its float bits copied.  Otherwise
 *   mean = (double)[1..3] / ((double)count 2^32); A, b = (double)[5..13] / 2^36, tr = (A00 + A11) + A22; contraction average
 *   or tr == 0: x = mean; else x solves (A + mu I) x = mu mean - b, mu = regularization tr (any direct float64 3x3 method:
 *   the eigenvalues of A lie in [0, tr], so the matrix is symmetric positive definite with condition <= (1 + reg) / reg);
 *   x clamped to [-0.5, 0.5] per axis; out = (float)(lo + h ((c + 0.5) + x)): a representative never leaves its cell.
 * Triangles: corners -> clusters; dropped with two equal corners; rotated so that the smallest cluster comes first
 *   (orientation kept); among equal rotated triples the lowest input index stays; emitted in ascending input index.  The
 *   same three clusters in the opposite orientation are another triangle.
 * Vertices out: the clusters a kept triangle references, in ascending cell id; vertex_map int[V] = the output index of each
 *   input vertex's cluster, -1 if it has none.
 * ishap_mesh_simplify_count: counts int[3] (device) = {vertices out, triangles out, status}; the first two ints of `scratch`
 *   then hold {clusters, triangles with three distinct clusters}.  ishap_mesh_simplify_emit: same arguments and the SAME
 *   scratch, untouched in between; out_verts float[3 vertices], out_tris int[3 triangles], vertex_map int[V];
 *   vertex_cluster: NULL, or int[V] that receives the cluster of every input vertex (the partition itself; -1 for an empty mesh).
 *   contraction: 0 quadric, 1 average.  scratch: ishap_mesh_simplify_scratch_bytes(V, F, dims) (-1 on bad sizes), 16-byte
 *   aligned: the cell bitmap and its ranks (2 x 4 bytes per 32 cells), 4 bytes per vertex, 132 per possible cluster
 *   (min(V, cells)), the triangle table (a power of two >= 2 F words) and 4 bytes per triangle.
 *   Refused with -2 and a message before anything is enqueued: a NULL pointer, h <= 0 or not finite, a dim < 1, more than 2^30
 *   cells, a scratch too small, an unknown contraction, 3 F or V beyond int32.  F = 0 or V = 0: an empty mesh (counts 0,
 *   vertex_map -1), set by memsets, no kernel launch.  lo and dims are HOST pointers, read during the call. */
long long ishap_mesh_simplify_scratch_bytes(long long nverts, long long ntris, const int* dims);
int ishap_mesh_simplify_count(const float* verts, long long nverts, const int* tris, long long ntris, const double* lo, double h,
                              const int* dims, int contraction, void* scratch, long long scratch_bytes, int* counts, void* stream);
int ishap_mesh_simplify_emit(const float* verts, long long nverts, const int* tris, long long ntris, const double* lo, double h,
                             const int* dims, int contraction, double regularization, void* scratch, long long scratch_bytes,
                             float* out_verts, int* out_tris, int* vertex_map, int* vertex_cluster, void* stream);

/* in place: v <- (v + sum of neighbours) / (1 + number of neighbours), `iterations` Jacobi sweeps (each neighbour once:
 * Open3D's filter_smooth_simple).  box_max > 0: the vertices are in grid coordinates of a [0, box_max]^3 volume and the
 * mesh may be open where the surface leaves the box (edges lying in a box face belong to one triangle); box_max <= 0: the
 * mesh is closed.  scratch: ishap_mesh_smooth_scratch_bytes(nverts, ntris) device bytes (the vertex adjacency, built once per
 * call, and a second vertex buffer; ~28 bytes per vertex + 24 per triangle).  Vertex indices and 6*ntris must fit 32 bits. */
long long ishap_mesh_smooth_scratch_bytes(long long nverts, long long ntris);
/* ABI version 2: `scratch_bytes` = the size of the caller's buffer; a buffer smaller than
 * ishap_mesh_smooth_scratch_bytes(nverts, ntris) fails the call (version 1 took 32 * nverts bytes on trust). */
int ishap_mesh_smooth(float* verts, long long nverts, const int* tris, long long ntris, int iterations, float box_max,
                      void* scratch, long long scratch_bytes, void* stream);
/* out2[0] = mean over a of min_b |a-b|^2, out2[1] = mean over b of min_a |a-b|^2 (device floats; their sum is the
 * reference's chamfer distance); nearest: device scratch float[max(na, nb)] */
int ishap_chamfer(const float* a, long long na, const float* b, long long nb, float* nearest, float* out2, void* stream);

/* ------------------------------------------------------------------ occupancy samples of an input mesh (8(f) rank 2)
 * Replaces the Open3D calls of train_triplane's data preparation (drag_utils.py:411-440): mesh.sample_points_uniformly
 * (area-weighted triangle choice -- the caller draws the triangle indices from `areas` and the uniforms) and
 * RaycastingScene.compute_occupancy (here: parity of the crossings of the +x ray with the closed triangle mesh).
 * verts: device float[3*nverts]; tris: device int[3*ntris]. */
int ishap_mesh_tri_areas(const float* verts, const int* tris, long long ntris, float* areas, void* stream);
/* pts[i] = uniform point of triangle tri_idx[i] from the uniforms uw[2i], uw[2i+1] */
int ishap_mesh_points_on_tris(const float* verts, const int* tris, const int* tri_idx, const float* uw, long long n,
                              float* pts, void* stream);
/* occ[i] = 1 inside / 0 outside */
int ishap_mesh_occupancy(const float* verts, const int* tris, long long ntris, const float* pts, long long npts,
                         float* occ, void* stream);

/* ------------------------------------------------------------------ mesh metrics (meshProcess.py:7-118)
 * Replaces the reference's Open3D RaycastingScene / cKDTree queries behind calc_implicit_field, calc_hausdorff, calc_iou,
 * calc_local_distance and calc_mesh_points_normals.
 * dist[i] = distance from pts[i] to the nearest triangle (exact fp32 closest point: vertex, edge and face regions), signed
 * when sdf != 0: negative inside, inside by the +x ray parity of ishap_mesh_occupancy (sdf == 2, ABI 12: inside where the
 * winding number of ishap_mesh_winding exceeds 0.5 -- the sign survives holes, doubled faces and interior sheets; the
 * mesh is counter-clockwise seen from outside, sdf == -2 is the same for a clockwise mesh: inside where w < -0.5); tri[i] = the nearest triangle, the
 * lowest index on exact ties (may be null).  Deterministic.  scratch: ishap_mesh_distance_scratch_bytes(ntris) device
 * bytes (one box per tile of 256 triangles, 32 bytes each); ntris < 2^31.  sdf == 2 / -2 needs the larger
 * ishap_mesh_distance_scratch_bytes_sdf(ntris, npts, 2) (the boxes, then the winding number's part sums); for every other sdf
 * (0: unsigned; any other value: parity, as 1) that function returns ishap_mesh_distance_scratch_bytes(ntris).  Both return -1 on invalid sizes. */
long long ishap_mesh_distance_scratch_bytes(long long ntris);
long long ishap_mesh_distance_scratch_bytes_sdf(long long ntris, long long npts, int sdf);
int ishap_mesh_distance(const float* verts, const int* tris, long long ntris, const float* pts, long long npts, int sdf,
                        float* dist, int* tri, void* scratch, long long scratch_bytes, void* stream);
/* out2[0] = max over a of min_b |a-b|^2, out2[1] = max over b of min_a |a-b|^2 (squared Hausdorff distances, device floats);
 * nearest: device float[na + nb], left holding the per-point minima (a's first) */
int ishap_hausdorff(const float* a, long long na, const float* b, long long nb, float* nearest, float* out2, void* stream);
/* fa, fb: device float[groups * per_group], two fields on the same samples, group-major.  out: device float[2*groups + 2]:
 * out[g] = |A and B| / |A or B| of group g (inside: value < 0, or value != 0 when `occupancy`; NaN for an empty union),
 * out[groups + g] = mean of (fb - fa)^2, out[2*groups] / out[2*groups + 1] = their means over the groups.  Fixed summation
 * order, double accumulators: bitwise repeatable. */
int ishap_group_field_stats(const float* fa, const float* fb, int groups, long long per_group, int occupancy, float* out,
                            void* stream);

/* ------------------------------------------------------------------ generalized winding number (ABI 12)
 * Inside / outside that does not need a closed surface: the reference's data preparation assumes watertight meshes
 * (drag_utils.py:437-440) or starts from oriented point clouds (meshProcess.py cloud2mesh: pointcloud.npz with `points` and
 * `normals`).  Brute force over (query, primitive) pairs, fp32, compensated sums.
 * ishap_mesh_winding: w[q] = 1/(4 pi) sum_f Omega_f(q), Omega by van Oosterom-Strackee (Jacobson et al. 2013): exactly 1
 *   inside / 0 outside a closed mesh whose triangles are counter-clockwise seen from outside (-1 inside when they are
 *   clockwise), k inside k nested copies, and a smooth value in between where the surface is open.  A triangle without
 *   area contributes 0.
 * ishap_cloud_winding: w[q] = 1/(4 pi) sum_i areas[i] (points[i] - q) . normals[i] / r^3 with
 *   r^2 = max(|points[i] - q|^2, areas[i] / (2 pi)) (Barill et al. 2018; the clamp bounds one sample's share by 1/2).
 *   normals: unit, outward.  areas: the surface area each sample stands for (ishap_cloud_areas, or the caller's own).
 * ishap_cloud_areas: areas[i] = max(pi d_k(i)^2 / k, 1e-12), d_k = distance to the k-th nearest OTHER point (points equal
 *   to point i count, at distance 0); 1 <= k <= 16, k < npoints.
 * With few queries the primitive range is split over workgroups; the part sums go to `scratch`
 * (ishap_winding_scratch_bytes(nprims, npts) device bytes, -1 on negative counts; a smaller scratch_bytes fails the call)
 * and are added in part order.  The split depends on (nprims, npts) only and there are no float atomics: a call repeats
 * bit for bit, and a query's value does not depend on where it stands in `pts`. */
long long ishap_winding_scratch_bytes(long long nprims, long long npts);
int ishap_mesh_winding(const float* verts, const int* tris, long long ntris, const float* pts, long long npts, float* w,
                       void* scratch, long long scratch_bytes, void* stream);
int ishap_cloud_winding(const float* points, const float* normals, const float* areas, long long npoints, const float* pts,
                        long long npts, float* w, void* scratch, long long scratch_bytes, void* stream);
int ishap_cloud_areas(const float* points, long long npoints, int k, float* areas, void* stream);

/* ------------------------------------------------------------------ clouds without normals (ABI 14)
 * What a scanner delivers is points only; the reference assumes its pointcloud.npz carries normals (a user of it would
 * call Open3D's estimate_normals and orient_normals_consistent_tangent_plane first).  Device pointers unless said otherwise;
 * 1 <= k <= 16 and k < npoints in all three calls; coordinates must be finite.
 * ishap_cloud_knn: idx[i*k + c], d2[i*k + c] = index and squared distance of the c-th nearest OTHER point of point i,
 *   ascending by (d2, index): equal distances go to the smaller index, points equal to point i are neighbours at distance 0.
 *   Brute force, fp32, npoints < 2^31.  A lane owns a query and the whole candidate range: the range is not split over
 *   workgroups, npoints / 256 workgroups are enough at the cloud sizes cloud_to_mesh is documented for (1e5 and up).
 *   Candidates are visited in a scattered tile order, so a cloud stored along a sweep costs no more than a shuffled one;
 *   the result does not depend on that order.
 * ishap_cloud_normals: normals[i] = the unit eigenvector of the smallest eigenvalue of the covariance of {point i} + its k
 *   neighbours idx[i*k ..] about their mean (coordinates relative to point i; covariance and cyclic Jacobi in fp64, rounded once to fp32), signed so that its
 *   component of largest magnitude is positive (ties: the lowest axis): a function of the input alone, NOT an orientation.
 *   variation (may be NULL): l0 / (l0 + l1 + l2), 0 on a plane.  All points equal: (1, 0, 0) and 0; collinear points: some
 *   unit vector across the line.  An index outside [0, npoints) is read as the point itself.
 * ishap_cloud_orient: flips normals (in place; each comes out as it went in or negated, bit for bit) so that they agree
 *   along the directed kNN graph.  Round r: every point that has no level yet takes, among its OWN neighbours with a level
 *   in [1, r), the one with the largest |n_i . n_j| (ties: the first in neighbour order), is negated where that dot product
 *   is negative (zero counts as positive) and gets level r.  A round that orients nothing while points remain makes the
 *   remaining point with the largest z (ties: the smallest index) a seed of level r, negated where n_z < 0; round 1 always
 *   seeds.  The topmost point of a closed surface that is not nested inside another has an outward normal with n_z > 0, so
 *   such components come out pointing OUTWARD; a cavity's surface nested inside another component comes out pointing away
 *   from its own interior, that is into the solid.  Independent of thread order, bitwise repeatable.
 *   info (HOST int[2]): the number of rounds in which propagation oriented at least one point, and the number of seeds.
 *   scratch: ishap_cloud_orient_scratch_bytes(npoints) device bytes (-1 on a negative count), 4-byte aligned; a smaller
 *   scratch_bytes fails the call.  npoints < 2^30 - 16.  Rounds are enqueued 16 at a time; the call synchronises the stream
 *   once per 16 rounds to read the number of points that remain, and has completed when it returns. */
int ishap_cloud_knn(const float* points, long long npoints, int k, int* idx, float* d2, void* stream);
int ishap_cloud_normals(const float* points, long long npoints, const int* idx, int k, float* normals, float* variation,
                        void* stream);
long long ishap_cloud_orient_scratch_bytes(long long npoints);
int ishap_cloud_orient(const float* points, float* normals, const int* idx, long long npoints, int k, void* scratch,
                       long long scratch_bytes, int* info, void* stream);

/* ------------------------------------------------------------------ ARAP deformation (meshProcess.py:222-236)
 * Replaces the reference's Open3D deform_as_rigid_as_possible: Sorkine & Alexa 2007, spokes energy, cotangent weights
 * w_ij = max(0, 1/2 sum cot) (triangles in ascending index), all arithmetic in fp64.  Device pointers throughout.
 * rest: float[nverts*3]; tris: int[ntris*3]; cons_ids: int[ncons], distinct, in [0, nverts); cons_pos: float[ncons*3].
 * out: float[nverts*3] (not aliasing rest): constrained vertices at their targets, vertices whose component of the w > 0
 * graph holds no constraint at rest (bit for bit), the free rest after max_iter alternations of the local rotation fit
 * and the global solve L_ff x_f = b_f - L_fc x_c (Jacobi-preconditioned CG on three columns, warm-started; a column stops
 * when |r| <= tol max(|rhs|, 1e-300) or after max_cg iterations, max_cg <= 0: 4 free vertices + 100).
 * energy: double[max_iter], E_k = sum_i sum_j w_ij |e'_ij - R_i e_ij|^2 at the rotations of step k and p'^(k-1);
 * cg_iters: int[max_iter], the CG iterations of step k, negated when max_cg ended the solve before every column met tol.
 * Triangle and constraint ids are checked on the device before use (an error names the fault).  Synchronises the stream
 * during setup and once per 32 CG iterations.  Bitwise repeatable.  scratch: ishap_arap_scratch_bytes device bytes. */
long long ishap_arap_scratch_bytes(long long nverts, long long ntris, long long ncons);
int ishap_arap(const float* rest, long long nverts, const int* tris, long long ntris, const int* cons_ids, const float* cons_pos,
               long long ncons, int max_iter, double tol, long long max_cg, float* out, double* energy, int* cg_iters,
               void* scratch, long long scratch_bytes, void* stream);
/* idx[i] = the vertex nearest to pts[i] (squared distance in fp64), the lowest index on ties (main.py:525-527's pick) */
int ishap_nearest_vertices(const float* verts, long long nverts, const float* pts, long long npts, int* idx, void* stream);

/* ------------------------------------------------------------------ connected components of a volume (ABI 16)
 * csrc/components.hip.  vol: float[nx*ny*nz], p = (x*ny + y)*nz + z (z fastest: the decoder's and ishap_surface_*'s layout),
 * the three extents independent.  A voxel is INSIDE where vol[p] - level > 0.f (the surface's own expression: a NaN is
 * outside), OUTSIDE otherwise.  nx*ny*nz must be below 2^31; a larger size, a non-positive extent, a connectivity other than
 * 6 or 26, a phase other than 0 or 1 or a null pointer returns -2 before anything is launched.  Device pointers throughout.
 *
 * ishap_volume_label: labels int[n].  phase 1 labels the inside voxels, phase 0 the outside voxels; voxels of the other phase
 * get -1.  Every labelled voxel gets THE LOWEST LINEAR INDEX OF ITS COMPONENT under connectivity 6 (face neighbours) or 26
 * (face, edge and corner neighbours): a function of the input alone, bitwise repeatable.  Three launches (union-find in LDS per
 * 4 x 8 x 32 tile, unions across tile seams, flatten); no kernel waits for another workgroup and the host reads nothing. */
int ishap_volume_label(const float* vol, int nx, int ny, int nz, float level, int phase, int connectivity, int* labels,
                       void* stream);
/* Device bytes of `scratch` for the three calls below on a volume of n voxels (-1 unless 0 < n < 2^31). */
long long ishap_volume_components_scratch_bytes(long long n);
/* The table of the components of `labels` (as ishap_volume_label wrote them), by the count / emit pattern of
 * ishap_surface_count / _emit: count writes the number of components C to count[0] (device int; the caller's one host
 * read-back) and leaves the root scan in `scratch`; emit, with the same labels and scratch, writes table int[C][9], one row per
 * component IN ASCENDING ROOT ORDER: root, voxels, xmin, xmax, ymin, ymax, zmin, zmax, border (1 when the component has a voxel
 * on any of the six faces of the box).  Integer sums and min / max: exact and repeatable.  Do not call emit when C == 0. */
int ishap_volume_components_count(const int* labels, int nx, int ny, int nz, void* scratch, int* count, void* stream);
int ishap_volume_components_emit(const int* labels, int nx, int ny, int nz, void* scratch, int* table, void* stream);
/* Every voxel whose label is in roots (device int[nroots]; entries outside [0, n) are ignored) is reflected across the level:
 * out = level - (in - level); a voxel moved to the inside whose mirror image would not be inside (in == level) gets the next
 * float above level.  Every other voxel, and every NaN voxel, is copied bit for bit.  vol_out may alias vol_in.  After the call
 * (out - level > 0) differs from the input's mask exactly on the non-NaN voxels of the listed components. */
int ishap_volume_flip(const float* vol_in, float* vol_out, const int* labels, int nx, int ny, int nz, float level,
                      const int* roots, long long nroots, void* scratch, void* stream);

/* ------------------------------------------------------------------ headless rendering (main.py:345-360, 492-507, 611-612)
 * Replaces what the reference asks of Open3D's scene widget: render_to_image, render_to_depth_image and camera.unproject.
 * The projection, coverage, depth and shading below are this library's OWN statement (csrc/render.hip; the fp64 form is
 * tests/render_ref.py); parity with Open3D's / Filament's pictures is unpinned.
 * Camera: looks from `eye` at `centre`; z_view > 0 in front of the eye; square pixels, f = (height/2) / tan(fov_y/2);
 * x_win = width/2 + f x_view / z_view, y_win = height/2 - f y_view / z_view (row 0 is the top of the picture). */
typedef struct {
  float eye[3], centre[3], up[3];
  float fov_y_deg, near, far;
} ishap_camera;
/* Device bytes ishap_render_mesh needs: 8 per pixel of visibility buffer + 16 per vertex + 16 per triangle + 16.
 * -1 for invalid sizes (negative or >= 2^31 counts, a picture side outside [1, 16384]). */
long long ishap_render_scratch_bytes(long long nverts, long long ntris, int width, int height);
/* Renders the triangle mesh (verts float[3*nverts], tris int[3*ntris], both windings drawn) into any of
 *   rgb    uint8 [height][width][3]  colour of the nearest triangle's part, background (0, 0, 0)
 *   depth  float [height][width]     d = far/(far-near) (1 - near/z_view) in [0, 1), background exactly 1.0f
 *   tri_id int   [height][width]     index of the nearest triangle, the lowest index on exact depth ties, background -1
 * (each may be null).  Coverage is sampled at pixel centres (x + 0.5, y + 0.5) with the top-left fill rule on window positions
 * rounded to 2^-14 pixel, in exact integer arithmetic: a closed mesh has no holes and no double hits along shared edges.
 * 1/z_view is interpolated perspective-correctly.  The result does not depend on the order of the triangles beyond their ids,
 * and two calls give the same bits.
 * NEAR PLANE: there is no clipping.  A triangle with ANY vertex nearer than `near` (z_view < near) is skipped whole, as is one
 * with a vertex more than 65536 pixels from the window origin, one of zero screen area, one whose bounding box holds no pixel
 * centre, and one with a vertex index outside [0, nverts).  Pixels at or beyond `far` are dropped.
 * normals: float[3*nverts] or null (flat face normals).  tri_part: int[ntris] or null (every triangle is part 0); parts:
 * float[4*nparts] rows (r, g, b, lit), colours in [0, 1].  Shading: rgb = colour * (0.25 + 0.75 |n . v|) when lit != 0, n the
 * normalised perspective-correctly interpolated normal and v the unit vector from the surface point to the eye (two-sided);
 * rgb = colour when lit == 0; then round(255 rgb).  parts is needed only with rgb.
 * scratch: 16-byte aligned device buffer of ishap_render_scratch_bytes(...) bytes; a smaller scratch_bytes fails the call. */
int ishap_render_mesh(const float* verts, long long nverts, const int* tris, long long ntris, const float* normals,
                      const int* tri_part, const float* parts, int nparts, const ishap_camera* camera, int width, int height,
                      void* scratch, long long scratch_bytes, unsigned char* rgb, float* depth, int* tri_id, void* stream);
/* camera.unproject(x, y, depth, width, height) (main.py:501-505): inverts the projection above for n rows (x, y, depth) of
 * xyd; x, y in pixels NAME THE PIXEL (its centre x + 0.5, y + 0.5 is unprojected), as the GUI's integer event.x / event.y do.
 * world: float[3*n].  Computed in fp64. */
int ishap_unproject(const ishap_camera* camera, int width, int height, const float* xyd, long long n, float* world, void* stream);

/* ------------------------------------------------------------------ measurement aid (bench.py roofline leg)
 * Brackets every implicit-GEMM launch with HIP events on its own stream between begin and end.
 * out[v*3+{0,1,2}] = {launches, total ms, algorithmic FLOPs}; one v per kernel symbol: 0 conv3x3 128^2 tile,
 * 1 conv3x3 64^2 tile, 2 GEMM 128^2 tile, 3 GEMM 64^2 tile, 4 conv3x3 64^2 tile two-team, 5 small-map GEMM kernel,
 * 6 register-staged stem kernel, 7 the 3x3 kernel's 128x32 halo tiles (csrc/igemm.hip lists 8-12; ishap_igemm_plan). */
int ishap_profile_begin(void);
int ishap_profile_end(double* out, int nvar);
/* Per-shape CSV ("M,N,K,conv3,tile,ksplit,launches,main_ms,reduce_ms,gflop" lines) of the same records; call
 * before the next ishap_profile_begin.  Returns the number of lines, -2 when `cap` is too small. */
int ishap_profile_shapes(char* buf, int cap);
/* The kernel choice of one convolution / GEMM launch, on the host, no GPU needed: the K split every layer launch gets (igemm_fill,
 * csrc/igemm.hip) and what igemm_launch then runs.  M = N*H*W output pixels (per batch entry), cin channels per tap, taps 9 (3x3) or 1, K2 channels of a
 * folded 1x1 second source, H x W the output map, pending: the consumer adds the K slices up, epilogue_sums: GroupNorm
 * statistics or GroupNorm-backward sums in the epilogue.  Writes the K split, the ishap_profile_end variant and the kernel
 * instance as a kernel trace names it (e.g. "igemm4_kernel<64, 64, 32, 4, 3, 1>").  0, or -2 when `kernel_cap` is too small. */
int ishap_igemm_plan(int M, int cin, int cout, int taps, int K2, int H, int W, int nbatch, int pending, int epilogue_sums,
                     int* ksplit, int* prof_slot, char* kernel, int kernel_cap);

/* One implicit-GEMM launch as a UNet layer makes it, for testing a kernel form in isolation (the call and the executor's
 * conv_op, csrc/unet.hip, describe the launch with the same record and fill their kernel arguments with the same function):
 *   out[m][n] = sum_k X(m, k) * Wt[n][k] (+ bias[n]) (+ bias2[n]) (+ res[m or its half-resolution pixel][n]),
 * k = tap * Cin + c over the 3x3 taps (zero padding per image; ups: the source map is (H/2, W/2), upsampled on the fly), then
 * K2 columns of the folded second source X2 against Wt columns [9 Cin, 9 Cin + K2).  The kernel form and the K split follow
 * from the shape exactly as in the product; the caller cannot choose them.  Every buffer comes with its size in bytes, and
 * every extent the launch would touch is checked against it (and its alignment) before any HIP call: a failed check returns
 * -2 with a message.  Row strides are in elements; X, X2, Wt, bias, bias2, ws and gb_x need 16-byte alignment, out and res
 * 8 bytes, and ldx, ldx2, ldw are multiples of 8, ldo and ldr multiples of 4. */
typedef struct {
  void* ptr;
  long long bytes;
} ishap_buf;
typedef struct {
  int M, N, Cin, taps, K2, H, W;   /* M = images * H * W output pixels, H x W the output map */
  int ldx, ldx2, ldw, ldo, ldr;
  int ups, res_ups;                /* X / the residual is the (H/2, W/2) map */
  int out_mode;                    /* 0: fp16 out[M][ldo]; 2: fp32 NCHW out[images][N][H][W] */
  int pending;                     /* the consumer adds the K slices up: with a K split they stay in ws (ishap_igemm_reduce) */
  int chunk_tiles;                 /* 0, or a multiple of 8: igemm4 forms run as launches of at most that many tiles */
  ishap_buf X;                     /* fp16 [pixels][ldx] */
  ishap_buf X2;                    /* fp16 [M][ldx2], K2 > 0 only */
  ishap_buf Wt;                    /* fp16 [round_up(N, 128)][ldw], rows >= N zero */
  ishap_buf out, bias, bias2;      /* bias, bias2: fp32 [N] or NULL */
  ishap_buf res;                   /* fp16 [M or M / 4][ldr] or NULL; may alias out */
  ishap_buf ws;                    /* fp32 [ksplit][M][N] when the launch splits K */
  ishap_buf stat_out;              /* int64 [images][N][2] or NULL: += (sum, sum of squares) of the stored values, fixed point */
  /* GroupNorm-backward sums (exclusive with stat_out): gb_csums [images][N][2] += (sum dyh, sum dyh * xhat), fixed point */
  ishap_buf gb_x, gb_stats, gb_gamma, gb_beta, gb_emb, gb_csums;
  int gb_emb_ld, gb_film, gb_act;
} ishap_igemm_desc;
/* Checks `d` and plans the launch; writes the K split and the kernel name (as ishap_igemm_plan does); with launch != 0 then
 * enqueues it on `stream` (the split-K reduce too, unless the slices are left pending).  launch = 0: no HIP call at all. */
int ishap_igemm_run(const ishap_igemm_desc* d, int launch, void* stream, int* ksplit, char* kernel, int kernel_cap);
/* The stand-alone reduce of a pending launch's `nslab` slices in d->ws into d->out (+ bias, bias2, res, res_ups): what a
 * consumer that cannot add slices up runs first (slab_materialize, csrc/unet.hip, through the same argument fill).  Reads M, N, H, W, ldo, ldr and those
 * buffers, checked as above; launch = 0: the checks only. */
int ishap_igemm_reduce(const ishap_igemm_desc* d, int nslab, int launch, void* stream);

/* One attention launch as a UNet AttentionBlock makes it (csrc/attention.hip), for testing a kernel form in isolation.
 * QKVAttentionLegacy per (image, head): a = softmax(q k^T / sqrt(d)) v, head h at qkv channels [h*3d, (h+1)*3d) as q | k | v.
 *   pass 0 (forward):  qkv -> out (a) and lse (log-sum-exp of each query's scores);
 *   pass 1 (backward): qkv, out, lse and dout (the gradient of a) -> dqkv.
 * T a multiple of 64, d = 32 or 64, C = heads * d.  The kernel form follows from the shape as in the product.  Every buffer is
 * checked against its size in bytes and its alignment (qkv, and in the backward out and dout, 16 bytes; out in the forward
 * and dqkv 8; lse 4) before any HIP call: a failed check returns -2 with a message. */
typedef struct {
  int pass;                        /* 0: forward, 1: backward */
  int N, T, C, heads, d;
  int xcd_map;                     /* -1: the product's setting (ISHAP_ATTN_XCD), 0: plain grid, 1: XCD-aware grid */
  ishap_buf qkv;                   /* fp16 [N][T][3C] */
  ishap_buf out;                   /* fp16 [N][T][C]: written by the forward, read by the backward */
  ishap_buf lse;                   /* fp32 [N * heads][T]: written by the forward, read by the backward */
  ishap_buf dout;                  /* fp16 [N][T][C], backward only */
  ishap_buf dqkv;                  /* fp16 [N][T][3C], backward only */
} ishap_attention_desc;
/* Checks `d` and writes the kernel instance (e.g. "attn_fwd_kernel<64,4>", "attn_bwd_kernel<32,2>/512" with its thread
 * count); with launch != 0 then enqueues it on `stream`.  launch = 0: no HIP call at all. */
int ishap_attention_run(const ishap_attention_desc* d, int launch, void* stream, char* kernel, int kernel_cap);

/* The 8x8-map AttentionBlock body (attn8_fused_kernel): qkv = xn Wqkv^T + bqkv, the attention of every head (d = 64, T = 64
 * tokens), and proj_out's K slice of each head, slices[h] = a_h Wproj[:, h*64 .. h*64+63]^T in fp32.  C = 64 * heads <= 1152,
 * and N * heads * 12 workgroups must fit on the device's compute units at once. */
typedef struct {
  int N, C, heads;
  ishap_buf xn;                    /* fp16 [N][64][C] */
  ishap_buf wqkv;                  /* fp16 [3C][C] */
  ishap_buf bqkv;                  /* fp32 [3C] */
  ishap_buf wproj;                 /* fp16 [C][C] */
  ishap_buf qkv;                   /* fp16 [N][64][3C], out */
  ishap_buf aout;                  /* fp16 [N][64][C], out */
  ishap_buf lse;                   /* fp32 [N][heads][64], out */
  ishap_buf slices;                /* fp32 [heads][N * 64][C], out */
  ishap_buf flags;                 /* uint32 [N][heads][16]: scratch, zeroed by the call */
} ishap_attention8_desc;
/* Checks `d` (launch = 0 stops there).  Otherwise fails on a pending device-side failure, zeroes the flags and enqueues the
 * block on `stream`: with one_launch != 0 as ONE launch whose workgroups wait for each other, if the device's rendezvous
 * tenancy is granted (*granted_out = 1), else as two launches of the same kernel (bitwise the same values).  A wait that gave
 * up is reported by the status check at the end of the call, or by the next call. */
int ishap_attention8_run(const ishap_attention8_desc* d, int one_launch, int launch, void* stream, int* granted_out);

#ifdef __cplusplus
}
#endif
#endif
