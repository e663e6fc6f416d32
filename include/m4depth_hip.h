/*
 * m4depth_hip.h -- C ABI of libm4depth_hip.so: the MI355X (gfx950) native
 * implementation of M4Depth's per-frame parallax-cost-volume inference path.
 *
 * This is the drop-in boundary.  The reference's only native interface is the
 * TensorFlow custom op pair BackProject / BackProjectGrad
 * (cuda_backproject/backproject_op.cc:32-42, launchers declared at
 * cuda_backproject/backproject_op_gpu.h:17-22); m4d_backproject_fwd/_bwd
 * replace those launchers one for one.  Every other entry point replaces a
 * piece of TF graph code of utils/depth_operations.py, utils/dense_image_warp.py
 * or m4depth_network.py:167-262 that the reference runs as dozens of unfused TF
 * ops; each declaration cites the lines it replaces.
 *
 * Conventions
 *   - all tensors are dense row-major NHWC float32 in device (HBM) memory unless
 *     a stride argument says otherwise; i = column (x), j = row (y);
 *   - the caller allocates every buffer; kernels never allocate, never retain
 *     pointers, write every output element (no memset dependency) and are
 *     enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream).  No host synchronisation; the calls are re-entrant,
 *     safe from several host threads on different streams, and hipGraph-capturable.
 *     The ONLY process-wide state is the table of environment switches, read once
 *     and never written again (m4d_switches_info), the launch counter
 *     (m4d_launch_count) and the DSCV kernel selector m4d_dscv_set_variant, the one
 *     setter of this library: the tests use it to run every DSCV kernel, the
 *     product's dispatch (m4depth_amd/network.py) never touches it, and it is not
 *     meant to be flipped while another thread launches.  Every tuning choice of the
 *     dispatch (which Winograd kernel, its staggered first round) is an ARGUMENT of
 *     the call.  No kernel of this library carries a profiling hook: the cycle-stamp
 *     buffers, the DSCV fallback counter, the measured-and-not-dispatched alternative
 *     kernels and the launch tape exist only in `make EXPERIMENTS=1`
 *     (include/m4depth_hip_experiments.h); the timing ablations are gone;
 *   - return value: 0 on success, otherwise a hipError_t code (1 =
 *     hipErrorInvalidValue for bad arguments).  Never exits the process (the
 *     reference launcher does `exit(-1)`, backproject_op_gpu.cu.cc:95-100);
 *   - `rot` is [b, rot_c] with rot_c = 4 (quaternion w,x,y,z, not renormalised)
 *     or 3 (small-angle x,y,z) as in get_rot_mat (utils/depth_operations.py:18-53);
 *     `trans` is [b,3]; `cam_f`, `cam_c` are the level-local intrinsics [b,2]
 *     (fx,fy) / (cx,cy) (m4depth_network.py:300-302);
 *   - arithmetic is IEEE float32 with one rounding per operation (the library is
 *     built with -ffp-contract=off) in the operand order of oracle/m4depth_oracle.py,
 *     so integer index grids are bit-exact against the oracle.
 */
#ifndef M4DEPTH_HIP_H_
#define M4DEPTH_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M4D_ABI_VERSION 6   /* 6: m4d_wino_set_stamps, m4d_wino6_set_stamps, m4d_front_set_stamps, m4d_dscv_set_stamps, m4d_dscv_set_fallback_counter (profiling hooks, never part of the reference surface) moved to m4depth_hip_experiments.h, - m4d_dscv_set_ablation (deleted with every other timing ablation); 6: + m4d_switches_info (the environment switches the library runs with; additive within ABI 6); 6: + m4d_train_log_step, m4d_train_log_workspace_bytes (device-side step log of the replayed training step; additive within ABI 6); 6: + m4d_depth_metrics_per_sample, m4d_metrics_per_sample_workspace_bytes (per-sample metrics of batched streaming evaluation; additive within ABI 6); 6 (round 6): + m4d_refiner_tail6_m, m4d_refiner_tail_m, m4d_level_post_m, m4d_stream_prepare (batched streaming inference with per-sample resets; additive, no existing entry point changed), m4d_normalize_levels, m4d_level_front_small(_supported) (a coarse level opens with ONE launch), m4d_conv3x3_wino6_bias_act_ks (the staggered first round as a per-launch argument), - m4d_wino6_set_stagger (process-wide state on the launch path), - m4d_conv3x3_lat_chain (measured 12.5 us per hand-over, never dispatched: deleted); 5 (round 5): + m4d_depth_metrics_strided, m4d_launch_count, m4d_conv3x3_lat, m4d_conv3x3s_lat, m4d_partial_finish, m4d_level_front_r, m4d_wino6_persistent_min_units, m4d_pack_conv_weights_lat, m4d_conv3x3_lat_chain, m4d_pyramid_reset(_supported), m4d_enc_level0_stats / _apply, m4d_wino6_set_stagger; 4 (round 4): + m4d_conv3x3_wino6_bias_act_k; the wino6 kernel selectors and the launch tape moved to m4depth_hip_experiments.h */

/* Library / device introspection (no GPU work). */
int m4d_abi_version(void);
/* Kernel launches this library has issued since it was loaded (host-side counter): the difference across one step -- or across
 * the hipGraph capture of one -- is the number of launches the step is made of (bench.py: roofline.launches_per_step). */
long long m4d_launch_count(void);
const char* m4d_build_info(void);
/* The environment switches of the library as this process read them (once, at the first call that needs one; never written
 * again): a static string "name=value" per switch, space separated -- "sncv_variant=1 sncv_ys=0 sncv_small_px=6000
 * wino_variant=4 wino4_min_wg=100 dscv_bwd_window_kb=48" with nothing set.  name = the variable without its M4D_ prefix, in
 * lower case; INTEGRATION.md lists them.  Additive entry point: ABI 6 unchanged. */
const char* m4d_switches_info(void);

/* ---- the reference's native op ------------------------------------------------ */

/* BackProjectForwardLauncher (backproject_op_gpu.cu.cc:83-103; kernel :19-79).
 * dims = {B,H,W,S,F,C} as built by BackProjectOp::Compute (backproject_op.cc:67-80).
 * input [B,H,W,F,C], coords [B,H,W,S,F,2] as (x,y), out [B,H,W,S,F,C].
 * Coordinates outside [0,W-1]x[0,H-1] produce zeros. */
int m4d_backproject_fwd(const float* input, const float* coords, const int dims[6],
                        float* out, void* stream);

/* BackProjectBackwardLauncher (backproject_op_gpu.cu.cc:201-223; kernel :108-197).
 * grad [B,H,W,S,F,C] -> input_grad [B,H,W,F,C] (fp32 atomic scatter, zero-filled by
 * the call itself), coords_grad [B,H,W,S,F,2]. */
int m4d_backproject_bwd(const float* grad, const float* input, const float* coords,
                        const int dims[6], float* input_grad, float* coords_grad, void* stream);

/* ---- utils/dense_image_warp.py -------------------------------------------------- */

/* dense_image_warp (:195-268) on its TF-CPU branch (_interpolate_bilinear, :61-192):
 * query = (j,i) + flow[(row,col)], floor clamped to [0,size-2], alpha to [0,1],
 * lerp form a*(r-l)+l.  image [B,H,W,C], flow [B,H,W,2] -> out [B,H,W,C].
 * index_out (may be NULL): int32 [B,H,W,2] = (y0,x0) -- the bit-exact index grid. */
int m4d_dense_image_warp(const float* image, const float* flow, int B, int H, int W, int C,
                         float* out, int32_t* index_out, void* stream);

/* _interpolate_bilinear (:61-192) with indexing='ij': grid [B,H,W,C], query [B,N,2] as
 * (row, col) -> out [B,N,C]; index_out (may be NULL) int32 [B,N,2] = (y0,x0). */
int m4d_interpolate_bilinear(const float* grid, const float* query, int B, int H, int W, int C,
                             int N, float* out, int32_t* index_out, void* stream);

/* ---- utils/depth_operations.py: converters -------------------------------------- */

/* parallax2depth (:141-166): depth = (s/disp - tz)/alpha.  disp,out [b,h,w,1]. */
int m4d_parallax2depth(const float* disp, const float* rot, int rot_c, const float* trans,
                       const float* cam_f, const float* cam_c, int b, int h, int w,
                       float* out, void* stream);
/* depth2parallax (:169-194): disp = s/(depth*alpha + tz). */
int m4d_depth2parallax(const float* depth, const float* rot, int rot_c, const float* trans,
                       const float* cam_f, const float* cam_c, int b, int h, int w,
                       float* out, void* stream);
/* prev_d2para (:197-215); rot is accepted for signature parity and ignored. */
int m4d_prev_d2para(const float* prev_d, const float* rot, int rot_c, const float* trans,
                    const float* cam_f, const float* cam_c, int b, int h, int w,
                    float* out, void* stream);
/* The flow field reproject (:72-105) hands to dense_image_warp plus its two auxiliary
 * outputs.  depth [b,h,w,1] -> flow [b,h,w,2] (row,col), proj_minus_rot [b,h,w,2],
 * rot_coord [b,h,w,2] (either aux pointer may be NULL). */
int m4d_reproject_flow(const float* depth, const float* rot, int rot_c, const float* trans,
                       const float* cam_f, const float* cam_c, int b, int h, int w,
                       float* flow, float* proj_minus_rot, float* rot_coord, void* stream);
/* recompute_depth (:109-137). */
int m4d_recompute_depth(const float* depth, const float* rot, int rot_c, const float* trans,
                        const float* cam_f, const float* cam_c, int b, int h, int w,
                        float* out, void* stream);

/* ---- utils/depth_operations.py: cost volumes ------------------------------------ */

/* get_parallax_sweeping_cv, the DSCV (:224-281).
 * c1, c2 [b,h,w,C]; disp_prev_t, disp [b,h,w,1]; nbre_cuts divides C.
 * cv: channel kk*(2r+1)+(n+r) of pixel p is written at cv[p*cv_stride + kk*(2r+1)+(n+r)]
 *     (cv_stride >= k*(2r+1); pass k*(2r+1) for a dense [b,h,w,k*(2r+1)] tensor, or the
 *     refiner-input width to write straight into f_input).  Products are formed in
 *     float16 and averaged per cut (cv_accum: 0 = float32 sum, one rounding to half;
 *     1 = sequential half adds) as at :276-277.
 * prev_disp (may be NULL) [b,h,w,2r+1]: the warped disp_prev_t channel (:273,:280).
 * log_center (may be NULL): writes log(prev_disp[...,r] * log_scale) at
 *     log_center[p*log_stride] -- the time-recurrence feature of m4depth_network.py:238.
 * index_out (may be NULL): int32 [b,h,w,2r+1,2] = (y0,x0) of every hypothesis. */
int m4d_dscv_fwd(const float* c1, const float* c2, const float* disp_prev_t, const float* disp,
                 const float* rot, int rot_c, const float* trans, const float* cam_f,
                 const float* cam_c, int b, int h, int w, int C, int search_range, int nbre_cuts,
                 int cv_accum, float* cv, int cv_stride, float* prev_disp,
                 float* log_center, int log_stride, float log_scale,
                 int32_t* index_out, void* stream);

/* The kernel selector of the DSCV (process-wide, not part of the reference surface; bit-identical results):
 * variant 0 = generic kernel, 1 = wave kernel with global gathers (default: fastest measured),
 * 2 = LDS search-window kernel, 3 / 4 = LDS window with 3 / all hypotheses per lane. */
void m4d_dscv_set_variant(int variant);

/* cost_volume, the SNCV (:284-313): out channel ((y*(2r+1)+x)*k + kk) =
 * leaky_relu(mean_c c1[j,i,c] * c2pad[j+y*d, i+x*d, c], 0.1), written at
 * out[p*out_stride + channel]. */
int m4d_sncv_fwd(const float* c1, const float* c2, int b, int h, int w, int C, int search_range,
                 int dilation_rate, int nbre_cuts, float* out, int out_stride, void* stream);
/* m4d_dscv_fwd and m4d_sncv_fwd(c1, c1, ...) of one level (depth_operations.py:224-281 and :284-313 as called from
 * m4depth_network.py:220-233).  On small maps (the coarsest pyramid levels) the two independent volumes share ONE launch --
 * one kernel boundary less on the coarse-level latency chain; otherwise the two entries are called one after the other.
 * Same results, bit for bit. */
int m4d_dscv_sncv_fwd(const float* c1, const float* c2, const float* disp_prev_t, const float* disp,
                      const float* rot, int rot_c, const float* trans, const float* cam_f,
                      const float* cam_c, int b, int h, int w, int C, int search_range, int nbre_cuts,
                      int cv_accum, float* cv, int cv_stride, float* prev_disp,
                      float* log_center, int log_stride, float log_scale,
                      int sncv_search_range, float* sncv_out, int sncv_out_stride, void* stream);

/* The same stride-1 layer by Winograd F(2x2,3x3) on the fp32 matrix cores: 2.25x fewer multiply-adds, result
 * equal to the direct convolution up to float32 rounding (the transforms only add and halve).  wu = the filter
 * transformed on the host, U = G g G^T, packed [ceil(Cin/16)][16 positions][CoutPad][16 channels]
 * (network_ops.pack_conv_weights_winograd); CoutPad a multiple of 32.  Deterministic. */
int m4d_conv3x3_wino_bias_act(const float* x, const float* wu, const float* bias, int b, int h, int w,
                              int Cin, int Cout, int CoutPad, float slope, float* out, void* stream);
/* Variant with half the weight traffic per flop (16x16-pixel workgroup tile, 8-channel K chunks): wu8 packed
 * [ceil(Cin/8)][16 positions][CoutPad][8 channels]; Cin % 4 == 0, x 16-byte aligned. */
int m4d_conv3x3_wino2_bias_act(const float* x, const float* wu8, const float* bias, int b, int h, int w,
                               int Cin, int Cout, int CoutPad, float slope, float* out, void* stream);
/* The same convolution with float32 operands on the BF16 matrix cores: every float32 operand is the exact sum of three
 * bf16 terms, six of the nine term products are accumulated in float32 (the dropped ones are below float32's product
 * rounding): float32 accuracy at 2.67x less matrix-core time.  wu6 = the transformed filter split and packed on the host
 * (network_ops.pack_conv_weights_wino6: [Cin/16][CoutPad/64][16][2][3][64][8] bf16); Cin % 16 == 0, CoutPad % 64 == 0.
 * Replaces the same tf.keras Conv2D + leaky_relu pairs as m4d_conv3x3_wino2_bias_act (m4depth_network.py:101-131). */
int m4d_conv3x3_wino6_bias_act(const float* x, const void* wu6, const float* bias, int b, int h, int w,
                               int Cin, int Cout, int CoutPad, float slope, float* out, void* stream);
/* The same call with the kernel named: 0 = chosen from the grid (what m4d_conv3x3_wino6_bias_act does), 1 = one workgroup
 * per (16x16-pixel tile, 64 output channels) (csrc/m4d_wino6.hip), 2 = persistent workgroups, one per CU, each walking a
 * contiguous range of (tile, cout group) units with the DMA stream continuing across unit boundaries (csrc/m4d_wino6p.hip;
 * Cin >= 32); 16 + n (1 <= n <= 15, round 6) = persistent workgroups of n CONSECUTIVE units each (n = 2 on a 128-cout layer: a
 * tile's two cout groups, one halo fetch, one unit boundary with the DMA stream running through it), as many workgroups as that
 * takes -- the dispatcher places them as CUs free instead of one static range per CU.  Bit-identical results; an argument, not
 * process state: tests and A/B timing use it. */
int m4d_conv3x3_wino6_bias_act_k(const float* x, const void* wu6, const float* bias, int b, int h, int w,
                                 int Cin, int Cout, int CoutPad, float slope, float* out, int kernel, void* stream);
/* Grids of at least this many (16x16-pixel tile, 64-cout) units run on the persistent-workgroup form of the kernel above when
 * `kernel` is 0 (what bench.py needs to name the kernel its roofline layer ran on). */
long long m4d_wino6_persistent_min_units(void);
/* The same call with a STAGGERED FIRST ROUND as well (ABI 6; replaces round 5's process-wide m4d_wino6_set_stagger): with
 * stagger_us > 0 the one-workgroup-per-unit kernel starts its first 256 workgroups (one per CU) in stagger_phases groups (a
 * power of two <= 32) spread over stagger_us microseconds (<= 1000): identical workgroups would otherwise free every CU at the
 * same instant once per unit time, and the small kernels of another frame's coarse levels wait for that instant
 * (csrc/m4d_wino6.hip).  A per-launch argument like `kernel`: nothing is remembered between calls, two callers with different
 * settings never see each other's (tests/test_gpu_ops.py::test_winograd_stagger_is_per_call).  Ignored by the persistent
 * kernel; results are the same bits either way.  Which launches should carry it is the caller's policy (network.py: grids of
 * >= 200 workgroups at batch <= 4; whether it pays depends on the box). */
int m4d_conv3x3_wino6_bias_act_ks(const float* x, const void* wu6, const float* bias, int b, int h, int w,
                                  int Cin, int Cout, int CoutPad, float slope, float* out, int kernel,
                                  int stagger_us, int stagger_phases, void* stream);
/* The same convolution with every float32 operand split into TWO fp16 terms after a power-of-two scale (per Winograd tile
 * for the input, per output channel for the weights), three fp16 MFMA products per term pair, float32 accumulation
 * (csrc/m4d_wino_f16.hip; error against float64 at the level of the bf16 three-term split).  wuh = network_ops.
 * pack_conv_weights_winof16: [Cin/16][CoutPad/64][16][2][2][64][8] fp16 followed by [CoutPad] int16 weight exponents.
 * One workgroup per (16x16-pixel tile, 64 output channels) at every grid size; stagger_us / stagger_phases as in
 * m4d_conv3x3_wino6_bias_act_ks.  Additive entry point: ABI 6 unchanged. */
int m4d_conv3x3_winof16_bias_act_ks(const float* x, const void* wuh, const float* bias, int b, int h, int w,
                                    int Cin, int Cout, int CoutPad, float slope, float* out,
                                    int stagger_us, int stagger_phases, void* stream);
/* The same call in a CHAIN of such layers: the kernel derives its input scales from the largest finite |x| of every input pixel,
 * which m4d_conv3x3_winof16_bias_act_ks finds by reading the halo of every unit once more, and which the layer that wrote x had
 * in registers.  pm_out (or NULL): uint32 [b][h][w][CoutPad/64], written by this call -- per pixel and group of 64 output
 * channels the largest min(bits(|y|), 0x7f7fffff) over the group's real channels of the values as stored (NaN counts as 0);
 * needs CoutPad - Cout < 64; every element is written, by plain stores.  pm_in (or NULL): uint32 [b][h][w][ceil(Cin/64)], the
 * pm_out of the call that wrote exactly this x (same b, h, w, Cout = this Cin) -- read instead of the scan.  Only the exponent
 * field of a maximum enters a scale, so outputs are the bits of the _ks call whenever pm_in holds the maxima of x (to the
 * exponent); with both NULL this IS the _ks call.  Both 4-byte aligned, distinct.  Additive entry point: ABI 6 unchanged. */
int m4d_conv3x3_winof16_bias_act_pm(const float* x, const void* wuh, const float* bias, int b, int h, int w,
                                    int Cin, int Cout, int CoutPad, float slope, float* out,
                                    const unsigned* pm_in, unsigned* pm_out,
                                    int stagger_us, int stagger_phases, void* stream);

/* The tail of a level in one kernel: the last two DispRefiner convolutions (32 -> 16 + leaky_relu(0.1), 16 -> 5;
 * m4depth_network.py:109-135) and m4d_level_post (:247-260).  x32 [b,h,w,32]; w6p [9][16][32] = kernel[ky][kx][k][n] as
 * [tap][n][k]; w7p [9][16][16] likewise with rows n >= 5 zero; outputs as m4d_level_post. */
int m4d_refiner_tail(const float* x32, const float* w6p, const float* b6, const float* w7p, const float* b7,
                     const float* rot, int rot_c, const float* trans, const float* cam_f, const float* cam_c,
                     int b, int h, int w, float scale, float* parallax, float* depth, float* other,
                     float* depth_state, void* stream);
/* The same tail with float32 operands split exactly into three bf16 terms on the bf16 matrix cores (csrc/m4d_tail6.hip; the
 * arithmetic of m4d_conv3x3_wino6_bias_act), persistent workgroups over 14x10-pixel tiles.  w6f / w7f = the B fragments of
 * network_ops.pack_refiner_tail_weights6: [9 taps][3 parts][64 lanes][8 bf16] with lane = (k-quarter, cout) holding input
 * channels 8 kq .. 8 kq + 7, and [5 K-steps][3 parts][4 k-quarters][8 couts][8 bf16] with k-quarter kq holding channels
 * 8 (kq & 1) .. + 7 of tap 2 j + (kq >> 1) (zeros for the tenth tap and couts 5..7). */
int m4d_refiner_tail6(const float* x32, const void* w6f, const float* b6, const void* w7f, const float* b7,
                      const float* rot, int rot_c, const float* trans, const float* cam_f, const float* cam_c,
                      int b, int h, int w, float scale, float* parallax, float* depth, float* other,
                      float* depth_state, void* stream);

/* ---- streaming inference: B independent streams in one batch, per-sample trajectory resets on the device ---------------------
 * The masked level close: m4d_refiner_tail6 / m4d_refiner_tail / m4d_level_post with reset [b] (uint8, nonzero = the sample's
 * trajectory starts at this frame).  A masked sample gets the reset constants m4d_pyramid_reset writes (m4depth_network.py:198-214):
 * parallax = reset_parallax (the caller passes 2^(number of coarser levels)), depth = 1000, other = 0, depth_state = 1000 -- the
 * refiner's values are neither computed nor written for it; an unmasked sample gets exactly the bits of the unmasked entry point
 * (:216-260).  depth_state and reset are required here.  No sample's result depends on another sample's inputs. */
int m4d_refiner_tail6_m(const float* x32, const void* w6f, const float* b6, const void* w7f, const float* b7,
                        const float* rot, int rot_c, const float* trans, const float* cam_f, const float* cam_c,
                        int b, int h, int w, float scale, float* parallax, float* depth, float* other,
                        float* depth_state, const unsigned char* reset, float reset_parallax, void* stream);
int m4d_refiner_tail_m(const float* x32, const float* w6p, const float* b6, const float* w7p, const float* b7,
                       const float* rot, int rot_c, const float* trans, const float* cam_f, const float* cam_c,
                       int b, int h, int w, float scale, float* parallax, float* depth, float* other,
                       float* depth_state, const unsigned char* reset, float reset_parallax, void* stream);
int m4d_level_post_m(const float* refiner_out, const float* rot, int rot_c, const float* trans,
                     const float* cam_f, const float* cam_c, int b, int h, int w, float scale,
                     float* parallax, float* depth, float* other, float* depth_state,
                     const unsigned char* reset, float reset_parallax, void* stream);
/* One launch per streamed frame (the reference's per-frame loop, main.py:150-172, with the batch-level rule of
 * m4depth_network.py:206-208 made per sample): reset[s] = force_all || new_traj[s] (new_traj [b] bool / uint8); rot_out [b,rot_c] /
 * trans_out [b,3] = the pose copy the level fronts read, in which a reset sample carries identity rotation ((0,0,0) small angle,
 * (1,0,0,0) quaternion) and translation (0,0,1) instead of its own (its outputs are the reset constants; its pose only keeps the
 * discarded arithmetic finite).  Continuing samples: their pose, unchanged. */
int m4d_stream_prepare(const unsigned char* new_traj, int force_all, const float* rot, int rot_c, const float* trans,
                       int b, unsigned char* reset, float* rot_out, float* trans_out, void* stream);

/* ---- gradients of the cost volumes (train_step, m4depth_network.py:371-399) ------ */

/* Backward of m4d_dscv_fwd: what tf.GradientTape derives from depth_operations.py:224-281.
 * g_cv: gradient of cv, read at g_cv[p*g_cv_stride + kk*(2r+1)+t]; g_prev_disp (may be NULL)
 * [b,h,w,2r+1]: gradient of the warped-parallax output.  The float16 product / mean (:276-278)
 * are differentiated in float16 as TF does; floor has no gradient and the two clip_by_value
 * pass inside their bounds (dense_image_warp.py:147-154, depth_operations.py:236).
 * Outputs: g_c1 [b,h,w,C], g_disp [b,h,w,1] (plain stores); g_c2 [b,h,w,C] and the optional
 * g_disp_prev_t [b,h,w,1] are scatter-adds (zero-filled by the call, float32 atomics: the
 * summation order varies run to run, as in BackProjectBackward, backproject_op_gpu.cu.cc:108-197).
 * C % 4 == 0, (C / nbre_cuts) % 4 == 0, C <= 256, 16-byte aligned feature pointers. */
int m4d_dscv_bwd(const float* c1, const float* c2, const float* disp_prev_t, const float* disp,
                 const float* rot, int rot_c, const float* trans, const float* cam_f,
                 const float* cam_c, int b, int h, int w, int C, int search_range, int nbre_cuts,
                 const float* g_cv, int g_cv_stride, const float* g_prev_disp,
                 float* g_c1, float* g_c2, float* g_disp, float* g_disp_prev_t, void* stream);

/* Backward of m4d_sncv_fwd (depth_operations.py:284-313).  out = the forward result (decides
 * the leaky_relu branch), g = its gradient, both read with their own pixel strides.
 * g_c1 / g_c2 [b,h,w,C] (either may be NULL); when c1 and c2 are the same map (the model's
 * auto-correlation, m4depth_network.py:232) the caller adds the two.  Deterministic. */
int m4d_sncv_bwd(const float* c1, const float* c2, const float* out, int out_stride,
                 const float* g, int g_stride, int b, int h, int w, int C, int search_range,
                 int dilation_rate, int nbre_cuts, float slope, float* g_c1, float* g_c2,
                 void* stream);

/* ---- per-pixel glue of the training graph (one kernel per autograd node) ----------- */

/* Adjoint of m4d_resize_bilinear_v1: g_out [b,oh,ow,c] -> g_in [b,ih,iw,c] (gather: deterministic). */
int m4d_resize_bilinear_v1_bwd(const float* g_out, int b, int ih, int iw, int c, int oh, int ow,
                               float mul, float* g_in, void* stream);
/* Backward of m4d_level_post (m4depth_network.py:247-251): gradients of parallax / depth / other
 * (any may be NULL = zero) -> gradient of the refiner output [b,h,w,5]. */
int m4d_level_post_bwd(const float* refiner_out, const float* g_parallax, const float* g_depth,
                       const float* g_other, const float* rot, int rot_c, const float* trans,
                       const float* cam_f, const float* cam_c, int b, int h, int w, float scale,
                       float* g_refiner_out, void* stream);
/* Backward of m4d_normalize_cuts: g_x = g/n - x * sum(g*x)/n^3 per cut. */
int m4d_normalize_cuts_bwd(const float* x, const float* g, int b, int h, int w, int C, int nbre_cuts,
                           float* g_x, void* stream);
/* Backward of the convolution epilogue leaky_relu(conv + bias): g_pre = g * (out > 0 ? 1 : slope)
 * (tf.nn.leaky_relu's gradient), g_bias[c] = sum over rows of g_pre (two-stage, fixed order).
 * workspace: m4d_bias_act_bwd_workspace_floats(rows, C) floats. */
long long m4d_bias_act_bwd_workspace_floats(long long rows, int C);
int m4d_bias_act_bwd(const float* g, const float* out, long long rows, int C, float slope,
                     float* g_pre, float* g_bias, float* workspace, void* stream);
/* Device-side weight packing for m4d_conv3x3*_bias_act*: w_ohwi = [O][3][3][I] (the channels-last
 * memory of an OIHW parameter) -> [ceil(K/16)][9][Npad][16]; transpose = 0: K = I, N = O (forward),
 * 1: K = O, N = I with the taps rotated by 180 degrees (data gradient of the stride-1 layer). */
int m4d_pack_conv_weights(const float* w_ohwi, int O, int I, int transpose, float* wp, void* stream);
/* ... in the layout of m4d_conv3x3_lat ([N/32][K/16][9][3 parts][64 lanes][8] bf16, every weight split exactly into three bf16
 * terms: what network_ops.pack_conv_weights_lat builds on the host), for the forward (transpose = 0: K = I, N = O) or the data
 * gradient (transpose = 1: the rotated / transposed kernel, K = O, N = I); wp: ceil(N/32) * ceil(K/16) * 27 KB. */
int m4d_pack_conv_weights_lat(const float* w_ohwi, int O, int I, int transpose, void* wp, void* stream);
/* One level's term of m4depth_loss (m4depth_network.py:491-536), unweighted:
 * mean |resize(log clip(gt)) - log clip(pred)| ('map': tf.image.resize bilinear, :532) or the
 * hole-aware block mean of velodyne ground truth (:514-527).  out2 = (term, point count);
 * workspace: m4d_loss_workspace_floats() floats.  Backward: g_pred [b,h,w,1] from the scalar
 * gradient g_out (device) and out2 of the forward. */
long long m4d_loss_workspace_floats(void);
int m4d_loss_level_fwd(const float* pred_depth, const float* gt_depth, int b, int h, int w, int H, int W,
                       int velodyne, float* workspace, float* out2, void* stream);
int m4d_loss_level_bwd(const float* pred_depth, const float* gt_depth, const float* stats2,
                       const float* g_out, int b, int h, int w, int H, int W, int velodyne,
                       float* g_pred, void* stream);

/* Step log of a (graph-replayed) training step, train_step's metric update (m4depth_network.py:418-427) without a host read:
 * RMSE_log of the last frame = sqrt(masked mean of (log(gt+1e-6) - log(est+1e-6))^2), mask log(gt+1e-6) > 1e-6, with gt
 * [b][H][W] (image stride gt_stride floats: a frame slice of the [b,T,H,W,1] batch) clamped to [0, 80] and est, the finest
 * estimate [b,h,w,1], resized to HxW by m4d_resize_nearest's index rule (inline) and clamped to [0.001, 80] (metrics.py:24-28).
 * Writes [*loss, rmse_log] to log[(*counter % log_rows) * 2 ..], then *counter += 1; sets *first_bad = the pre-increment
 * counter of the first non-finite loss (sticky: only while *first_bad < 0).  Block partials in double, fixed-order finish: the
 * same bits every run.  workspace: m4d_train_log_workspace_bytes() bytes. */
long long m4d_train_log_workspace_bytes(void);
int m4d_train_log_step(const float* loss, const float* gt, long long gt_stride, const float* est, int b, int H, int W,
                       int h, int w, float* log, int log_rows, long long* counter, long long* first_bad,
                       void* workspace, void* stream);

/* ---- Photometric reprojection loss: training without ground-truth depth (csrc/m4d_photo.hip) ----------
 * Standard self-supervised depth training (Godard et al., "Digging into self-supervised monocular depth estimation",
 * ICCV 2019, eq. 2-5: SSIM + L1 photometric error, auto-masking, edge-aware smoothness), one term per pyramid level, with the
 * exact relative pose of the data instead of a pose network.  Per level (map h x w) and frame t >= 1, with cur / prev the
 * level images of frames t / t-1 and dc = clip(depth, 0.01, 200):
 *   warped = reproject(prev, dc, rot, trans, camera)[0], bit for bit (the query and the bilinear sample of m4d_reproject_flow
 *            + m4d_dense_image_warp); valid = Pz > 0 and 0 <= qx <= w-1 and 0 <= qy <= h-1 and depth finite;
 *            dwarp = d warped / d dc, analytic: dq/ddc = (A Pz - Px C) / Pz^2 per axis, d warped/dqx = (1-ay)(tr-tl) + ay(br-bl),
 *            d warped/dqy = (1-ax)(bl-tl) + ax(br-tr), 0 on an axis whose alpha was clamped;
 *   pe(a,b) = 0.85 (1 - SSIM(a,b)) / 2 + 0.15 |a - b|, mean over the 3 channels, at interior pixels (1 <= y <= h-2,
 *            1 <= x <= w-2); SSIM over the 3x3 window, sigma^2 = mean(x^2) - mu^2, sigma_xy = mean(xy) - mu_x mu_y,
 *            C1 = 0.01^2, C2 = 0.03^2, no clipping;
 *   M(p)   = p interior and all 9 window pixels valid and (automask != 0: pe(warped,cur)(p) < pe(prev,cur)(p)); N = sum M;
 *   photo  = sum M pe(warped,cur) / max(N,1);
 *   smooth = [sum_{x<w-1} |ld(y,x+1) - ld(y,x)| exp(-mean_c |cur(y,x+1) - cur(y,x)|) + the same along y] / (b h w), ld = log dc;
 *   out4   = (photo + lambda smooth, photo, smooth, N).
 * Backward (a gather, no atomics): g_depth(q) = g_out * inside(q) * [ sum_c dwarp_c(q) sum_{p in 3x3(q)} M(p)
 *   d pe_c(p) / d warped_c(q) / max(N,1) + lambda d smooth / d dc(q) ], inside = (0.01 <= depth <= 200), with the mask and N
 *   of the forward.  Images are [b,h,w,3], depth / valid / mask [b,h,w,1] (valid, mask: one byte per pixel, 0 or 1); cameras
 *   are per sample and level-local; h, w >= 3, b h w <= 2^24.  Deterministic: block partials in double, fixed-order finish.
 *
 * Image pyramid (data, no gradient): level 0 = the 2x2 mean of image [n,H,W,3], ((a + b) + (c + d)) * 0.25 with a, b on the
 * upper row; level i = the same of level i-1.  Level i ([n, H >> (i+1), W >> (i+1), 3]) starts at float offset
 * sum_{k<i} n * 3 * (H >> (k+1)) * (W >> (k+1)) of `out`, which holds m4d_image_pyramid_floats floats (-1: H or W is no
 * multiple of 2^levels). */
long long m4d_image_pyramid_floats(int n, int H, int W, int levels);
int m4d_image_pyramid_box(const float* image, int n, int H, int W, int levels, float* out, void* stream);
int m4d_photo_warp_fwd(const float* depth, const float* rot, int rot_c, const float* trans, const float* cam_f,
                       const float* cam_c, const float* prev, int b, int h, int w, float* warped, float* dwarp,
                       unsigned char* valid, void* stream);
/* workspace of m4d_photo_loss_fwd in bytes (8-byte aligned); -1 for sizes the loss refuses */
long long m4d_photo_workspace_bytes(int b, int h, int w);
int m4d_photo_loss_fwd(const float* depth, const float* warped, const unsigned char* valid, const float* cur,
                       const float* prev, int b, int h, int w, float lambda, int automask, void* workspace,
                       float* out4, unsigned char* mask, void* stream);
int m4d_photo_loss_bwd(const float* depth, const float* warped, const float* dwarp, const float* cur,
                       const unsigned char* mask, const float* out4, const float* g_out, int b, int h, int w,
                       float lambda, float* g_depth, void* stream);

/* Full-resolution terms and the minimum over two sources (the two options of the loss; with scale = level and one source the
 * definition above, unchanged).  Frame t >= 1, level i, level depth d [b,h,w,1]:
 * Scale.  level: D = d, images and camera those of the level.  full: D = U_s(d), s = 2^(i+1), [b, h s, w s, 1]; the images
 *   are the input frames themselves (no pyramid), the camera the full-resolution one.  U_s = bilinear upsampling with
 *   half-pixel centres and edge clamp (PyTorch's interpolate(mode="bilinear", align_corners=False)); per axis, output index Y:
 *     src = max((Y + 0.5) / s - 0.5, 0), y0 = min(floor(src), h-1), y1 = min(y0 + 1, h-1), a = src - y0,
 *   value = m4d_lerp2(tl, tr, bl, br, ax, ay) in that operation order (s a power of two: src and a are exact in float32, the
 *   result is bit-reproducible).  The RAW depth is upsampled; the clip to [0.01, 200], `valid` and `inside` apply to D as
 *   they apply to `depth` above; smoothness is that of D against the full-resolution current image, divided by the number of
 *   elements of D.
 * Sources.  Source 0 = frame t-1 with the motion of frame t.  With two sources and t < T-1, source 1 = frame t+1 with the
 *   inverse of the motion of frame t+1: rot' = (w, -x, -y, -z), trans' = -(R(rot') trans); quaternions only (I + [r]x has no
 *   exact inverse of that form).  The last frame of a sequence has source 0 only.
 * Per source s: warped_s, dwarp_s, valid_s = m4d_photo_warp_fwd on D.  Per pixel p: pe_s(p) = pe(warped_s, cur)(p);
 *   ok_s(p) = p interior and all 9 window pixels valid for s; m(p), sel(p): walk the sources in order, source s replaces the
 *   choice when ok_s(p) and (nothing chosen yet or pe_s(p) < m(p)) -- a tie keeps the previous frame, no ok source selects
 *   nothing; id(p) = min over the present sources of pe(image_s, cur)(p) (independent of D: the same for every level of a
 *   frame at scale full); M(p) = sel(p) != none and (auto-masking off or m(p) < id(p)); N = sum M;
 *   photo = sum_M m / max(N,1); term and out4 as above.
 * Backward (a gather, no atomics): g_D(q) = g [ sum_s dwarp_s(q) sum_{p in 3x3(q), M(p), sel(p)=s} d pe_s(p)/d warped_s(q)
 *   / max(N,1) + lambda d smooth/dD(q) ] inside(q);  g_d = U_s^T g_D, the exact adjoint of U_s including the clamped border
 *   rows and columns, itself a gather: a coarse pixel collects from the at most 2s x 2s fine pixels whose stencil holds it, in
 *   a fixed order (s <= 4: one thread, row-major; s >= 8: one wave, lane l the values l, l+64, ..., double, shuffle tree).
 *
 * m4d_upsample_hp_*: x / g_x [b,h,w], out / g_out [b, h s, w s]; s in {2,4,8,16,32,64}, h, w >= 1, b (h s)(w s) <= 2^24,
 *   anything else: invalid argument, no launch.
 * m4d_photo_identity_fwd: pe_id [b,h,w] float32 = id above (src1 NULL: one source); non-interior pixels are written as 0 and
 *   never read.
 * m4d_photo_min_fwd: warped1 / valid1 NULL (both or neither) = one source; pe_id NULL = auto-masking off; sel [b,h,w] bytes,
 *   0 = not in M, 1 = previous, 2 = next; workspace of m4d_photo_min_workspace_bytes bytes, 8-byte aligned.
 * m4d_photo_min_bwd: one gather over both sources with the forward's sel and out4 (warped1 / dwarp1 NULL: one source, a sel
 *   byte of 2 then selects nothing). */
int m4d_upsample_hp_fwd(const float* x, int b, int h, int w, int s, float* out, void* stream);
int m4d_upsample_hp_bwd(const float* g_out, int b, int h, int w, int s, float* g_x, void* stream);
int m4d_photo_identity_fwd(const float* cur, const float* src0, const float* src1_or_null, int b, int h, int w, float* pe_id,
                           void* stream);
long long m4d_photo_min_workspace_bytes(int b, int h, int w);
int m4d_photo_min_fwd(const float* depth, const float* warped0, const unsigned char* valid0, const float* warped1,
                      const unsigned char* valid1, const float* cur, const float* pe_id, int b, int h, int w, float lambda,
                      void* workspace, float* out4, unsigned char* sel, void* stream);
int m4d_photo_min_bwd(const float* depth, const float* warped0, const float* dwarp0, const float* warped1, const float* dwarp1,
                      const float* cur, const unsigned char* sel, const float* out4, const float* g_out, int b, int h, int w,
                      float lambda, float* g_depth, void* stream);

/* ---- Reprojection consistency: a label-free score of the full-resolution estimate (csrc/m4d_consistency.hip) ----------
 * Scores the depth map a trajectory's frame was given against the previous frame of the same trajectory, without ground truth
 * (main.py --consistency).  Per sample s of a batch, at the input resolution H x W:
 *   D [H,W,1] the raw estimate of the current frame, Dp that of the previous frame; cur, prev [H,W,3] the two images;
 *   rot (rot_c 3 or 4), trans the current frame's motion (a point X of the current camera is R X + t in the previous one);
 *   cam_f, cam_c the sample's own full-resolution camera.
 * Warp.  (warped, valid, qx, qy, Pz) = the query of m4d_photo_warp_fwd on D, clip to [0.01, 200] and `valid` included: the
 *   same device functions in the same operation order (csrc/m4d_photo_common.h), the same bits; dwarp is not computed.
 * Photometric part.  M(p) = p interior and all 9 window pixels valid (no auto-mask); pe_w = pe(warped, cur)(p),
 *   pe_id = pe(prev, cur)(p) with pe and its double-precision window statistics as above; N = sum M.
 * Geometric part (the depth-consistency term of Bian et al., NeurIPS 2019).  G(p) = valid(p) and the four bilinear taps of Dp
 *   at the query are finite and > 0; Dq = m4d_lerp2 of those taps with the cell and alphas of the image sample;
 *   g(p) = |Pz - Dq| / (Pz + Dq) in double from the float32 Pz and Dq; Ng = sum G.
 * Row, six float32 values, each rounded once from double:
 *   photo = sum_M pe_w / N;  photo_id = sum_M pe_id / N;  better = #{p in M: pe_w < pe_id} / N;  geo = sum_G g / Ng;
 *   cover = N / ((H-2)(W-2));  geo_cover = Ng / (H W).
 * counted[s] = active[s] && !reset[s] && N > 0 && Ng > 0, decided on the device; a sample that is not counted gets a row of
 *   six zeros.  A sample with !active[s] || reset[s] has none of its images or depth maps read (its previous-frame buffers may
 *   hold another trajectory or nothing): its blocks leave after reading the masks.
 * Deterministic: block partials in double, wave64 shuffles, a fixed-order finish per sample, no atomics, no zero-fill (every
 *   block writes its own partial); row s of a batch launch equals the row of a launch on sample s alone bit for bit.
 * Layout: batch strides in floats (>= the dense image, H W or 3 H W), images dense: a frame slice of a [B,T,...] tensor is read
 *   in place.  reset, active: uint8 [b] device masks; rows6 [b][6] floats, counted [b] bytes; workspace of
 *   m4d_consistency_workspace_bytes(b, h, w) bytes, 8-byte aligned (-1: a size the call refuses).  Invalid argument, no launch:
 *   a NULL pointer, b outside [1, 65535], h or w < 3, h w > 2^24, rot_c not in {3,4}, a stride below the dense image, a
 *   workspace off 8 bytes.  Two plain launches (capturable).  Additive entry points: ABI 6 unchanged. */
long long m4d_consistency_workspace_bytes(int b, int h, int w);
int m4d_consistency_per_sample(const float* est, long long est_stride, const float* est_prev, long long est_prev_stride,
                               const float* cur, long long cur_stride, const float* prev, long long prev_stride,
                               const float* rot, int rot_c, const float* trans, const float* cam_f, const float* cam_c,
                               const unsigned char* reset, const unsigned char* active, int b, int h, int w, void* workspace,
                               float* rows6, unsigned char* counted, void* stream);

/* ---- Pose refinement: direct photometric alignment of the current frame against the previous one (csrc/m4d_align.hip) ----
 * Gauss-Newton image alignment (Lucas-Kanade on SE(3), as in direct visual odometry: Kerl et al., ICRA 2013; Engel et al.,
 * "Direct Sparse Odometry", 2018) started from the given motion (main.py --refine_pose).  Per sample: prev [H,W,3] and Dp
 * [H,W,1], the previous frame's image and raw estimate; cur [H,W,3]; rot (a unit quaternion, rot_c = 4 only; normalised in
 * double when it is read) and trans, the network's convention (a point X of the current camera is R X + t in the previous
 * one); cam_f, cam_c the sample's own full-resolution camera.  The pose is held as (A, a) = (R^T, -R^T t), the motion from the
 * previous camera (which has the depth) into the current one, in double on the device between iterations.
 * One iteration at a level of stride s (a power of two), level map h = H/s, w = W/s:
 *   images  grey = ((r + g) + b) / 3 of the box-pyramid level (m4d_image_pyramid_box; s = 1: the frames themselves);
 *   camera  f/s, c/s;  depth of level pixel (i, j) = Dp at full-resolution pixel (i s + s/2, j s + s/2), one tap, clipped to
 *           [0.01, 200]; a non-finite tap makes the pixel invalid;
 *   query   m4d_photo_query (csrc/m4d_photo_common.h) on the float32 rounding of (A, a): X = depth (x_n, y_n, 1) with the
 *           half-pixel centre, Y = A X + a, q = f Y.xy / Y.z + c - 0.5; valid = Y.z > 0, q inside [0,w-1] x [0,h-1], depth finite;
 *   residual r = bilinear(cur_level, q) - prev_level(p); image gradient = the analytic derivative of that sample,
 *           gx = (1-ay)(tr-tl) + ay(br-bl), gy = (1-ax)(bl-tl) + ax(br-tr);
 *   Jacobian for the left perturbation Y <- exp(w^) Y + v: g = dr/dY = (gx fx / Z, gy fy / Z, -(gx fx Yx + gy fy Yy) / Z^2),
 *           J = [g, Y x g] (translation first);  Huber weight wh = 1 if |r| <= huber else huber / |r|;
 *   per-pixel terms in float32 (one rounding per operation), products and sums in double over the valid pixels:
 *           H = sum wh J J^T (21 entries, upper triangle row-major), b = sum wh J r (6), cost = sum wh r^2, N;
 *   step    (H/N + damping diag(H/N) + W) delta = -(b/N + W xi_acc), 6x6 Cholesky in double; W = diag(prior_t x3, prior_r x3)
 *           a first-order prior towards the given pose, xi_acc the sum of the increments applied so far (0 = no prior);
 *   update  A <- exp(w^) A, a <- exp(w^) a + v, xi_acc += delta.  A pivot <= 0, N = 0 or a non-finite value marks the sample
 *           bad: its pose is left as it is and its later iterations do nothing.
 * End: R' = A^T, t' = -A^T a, the quaternion of R' normalised with w >= 0, each rounded to float32 once.  The result is
 *   rejected -- rot / trans written through bit for bit -- when reset[s] or !active[s] (none of the sample's images or maps is
 *   read, as in m4d_consistency_per_sample), the sample is bad, no iteration ran, N / (h w) of the last iteration is below
 *   min_cover, the cost/N of the last iteration is not below that of the first iteration at the same stride (both are taken
 *   before that iteration's update: a level needs two iterations to be accepted), |t' - t| > cap_t (metres) or the angle
 *   between R' and R > cap_r (radians).
 * rows8 [b][8]: cost/N at the first and at the last iteration of the last stride, N / (h w) there, |t' - t|, the angle, the
 *   iterations applied, the applied flag (1 / 0), 0; a masked-off sample's row is eight zeros.
 * Workspace: m4d_pose_align_workspace_bytes(b, H, W) bytes (-1: a size the calls refuse), 8-byte aligned, private to the
 *   frame between begin and end.  It opens with 64 doubles per sample that a caller may read: A (9, row-major), a (3),
 *   xi_acc (6), the first and last cost/N, N / (h w), iterations, the bad flag, the stride of the last iteration, 8 unused, then
 *   the folded sums of the last iteration (29: H, b, cost, N), 3 unused; the tile partials follow.
 * Deterministic: no atomics, no zero-fill, block partials in double (wave64 shuffles, LDS across waves), folded in index
 *   order by one wave per sample; sample s of a batch equals the launch on sample s alone bit for bit.  The decision is made
 *   on the device; nothing synchronises; every call is plain launches (begin 1, iterate 2, end 1), capturable.
 * Layout: batch strides in floats (>= the dense level image 3 h w, or H W for the estimate).  Invalid argument, no launch: a
 *   NULL pointer, rot_c != 4, b outside [1, 65535], H or W < 3, H W > 2^24, s no power of two, H or W no multiple of s, level
 *   h or w < 3, a stride below the dense image, huber <= 0, a negative damping / prior / min_cover / cap, a workspace off 8
 *   bytes.  Additive entry points: ABI 6 unchanged. */
long long m4d_pose_align_workspace_bytes(int b, int h, int w);
int m4d_pose_align_begin(const float* rot, int rot_c, const float* trans, int b, int h, int w, void* workspace, void* stream);
int m4d_pose_align_iterate(const float* cur, long long cur_stride, const float* prev, long long prev_stride,
                           const float* est_prev, long long est_prev_stride, const float* cam_f, const float* cam_c,
                           const unsigned char* reset, const unsigned char* active, int b, int h, int w, int s, float huber,
                           float damping, float prior_t, float prior_r, void* workspace, void* stream);
int m4d_pose_align_end(const float* rot, int rot_c, const float* trans, const unsigned char* reset, const unsigned char* active,
                       int b, int h, int w, float min_cover, float cap_t, float cap_r, const void* workspace, float* rot_out,
                       float* trans_out, float* rows8, void* stream);

/* ---- m4depth_network.py: DepthEstimatorLevel glue -------------------------------- */

/* Per-cut L2 normalisation (:179-189, tf.linalg.normalize, no epsilon). */
int m4d_normalize_cuts(const float* x, int b, int h, int w, int C, int nbre_cuts,
                       float* out, void* stream);

/* tf.compat.v1.image.resize_bilinear defaults (:202-204): x [b,ih,iw,c] -> out
 * [b,oh,ow,c], multiplied by `mul` (2.0 for the parallax map, :203). */
int m4d_resize_bilinear_v1(const float* x, int b, int ih, int iw, int c, int oh, int ow,
                           float mul, float* out, void* stream);
/* tf.image.resize(NEAREST_NEIGHBOR) (:368). */
int m4d_resize_nearest(const float* x, int b, int ih, int iw, int c, int oh, int ow,
                       float* out, void* stream);

/* Fused "preprocessor" glue of one level (:196-204, :218, :224-227):
 *   prev_l_* (coarser level estimate at [b,ph,pw,.]; all NULL at the coarsest level ->
 *   parallax 1, depth 1000, other 0) are x2-upsampled to para_prev_l [b,h,w,1] (x2),
 *   depth_prev_l [b,h,w,1], other_prev_l [b,h,w,4];
 *   para_prev_t [b,h,w,1] = prev_d2para(depth_prev_t) (skipped when depth_prev_t NULL);
 *   if f_input != NULL: f_input[p*f_stride + log_off] = log(para_prev_l * log_scale) and,
 *   when other_off >= 0, f_input[p*f_stride + other_off + 0..3] = other_prev_l;
 *   if depth_state_reset != NULL (the new_traj branch, :208-214): depth_state_reset [b,h,w,1] := 1000 (:209). */
int m4d_level_pre(const float* prev_l_depth, const float* prev_l_parallax, const float* prev_l_other,
                  int ph, int pw, const float* depth_prev_t, const float* trans,
                  const float* cam_f, const float* cam_c, int b, int h, int w,
                  float* para_prev_l, float* depth_prev_l, float* other_prev_l, float* para_prev_t,
                  float* f_input, int f_stride, int log_off, int other_off, float log_scale,
                  float* depth_state_reset, void* stream);
/* m4d_level_pre and m4d_normalize_cuts(norm_x -> norm_out) -- the two independent kernels that open a level
 * (m4depth_network.py:179-189 and :196-227) -- in ONE launch: one kernel boundary less on the coarse-level latency chain.
 * Same results, bit for bit. */
int m4d_level_pre_normalize(const float* prev_l_depth, const float* prev_l_parallax, const float* prev_l_other,
                            int ph, int pw, const float* depth_prev_t, const float* trans,
                            const float* cam_f, const float* cam_c, int b, int h, int w,
                            float* para_prev_l, float* depth_prev_l, float* other_prev_l, float* para_prev_t,
                            float* f_input, int f_stride, int log_off, int other_off, float log_scale,
                            float* depth_state_reset,
                            const float* norm_x, int C, int nbre_cuts, float* norm_out, void* stream);

/* The reset frame of a whole pyramid in ONE launch (m4depth_network.py:207-214 for every level of DepthEstimatorPyramid.call's
 * loop, :305-321, on a new trajectory): per level, prev_f_maps := the per-cut normalised features, depth_prev_t := 1000, and the
 * level's estimate -- the x2 upsampling chain of :202-204 started from the constants of :198-200, i.e. the constant maps
 * parallax = parallax_value (the caller passes 2^(number of coarser levels)), depth = 1000, other = 0.  Bit-identical to
 * m4d_level_pre_normalize called level by level, coarse to fine.  levels[] is read on the host during the call. */
typedef struct m4d_reset_level {
  const float* features;   /* [b,h,w,C] raw encoder features */
  float* state_features;   /* [b,h,w,C] <- normalised (becomes prev_f_maps) */
  float* depth_state;      /* [b,h,w,1] <- 1000 */
  float* parallax;         /* [b,h,w,1] <- parallax_value */
  float* depth;            /* [b,h,w,1] <- 1000 */
  float* other;            /* [b,h,w,4] <- 0 */
  int h, w, C, nbre_cuts;
  float parallax_value;
} m4d_reset_level;
int m4d_pyramid_reset_supported(int C, int nbre_cuts);      /* C / nbre_cuts in {8, 16, 24, 32} */
int m4d_pyramid_reset(const m4d_reset_level* levels, int n_levels, int b, void* stream);

/* The per-cut normalisation (tf.linalg.normalize per cut, m4depth_network.py:179-189) of up to 8 feature maps in ONE launch: the
 * normalised features of a frame depend on the encoder alone, so the coarse levels' maps of all frames of an encoder batch are
 * normalised right behind it, off the levels' latency chains (round 6).  x / out [pixels, C], pixels = frames * b * h * w; C /
 * nbre_cuts in {8, 16, 24, 32}.  The same bits as m4d_normalize_cuts. */
typedef struct { const float* x; float* out; long long pixels; int C, nbre_cuts; } m4d_norm_level;
int m4d_normalize_levels(const m4d_norm_level* levels, int n_levels, void* stream);
/* The opening of a COARSE level (maps <= 6000 pixels: levels 4-6 of the 384x1280 pyramid at batch 1) in ONE launch (round 6):
 * level_pre's glue + DSCV + SNCV of m4depth_network.py:196-242 on features that arrive per-cut normalised (norm_f [b,h,w,C]:
 * m4d_normalize_levels; it becomes prev_f_maps after the level, :211/:259).  [DSCV | SNCV | glue] workgroups of one grid, nothing
 * inside the launch depends on anything else in it: the DSCV evaluates the two maps the glue kernel would have written where it
 * needs them (para_prev_l = 2 x the x2 upsampling of the coarser level's parallax at its own pixel, prev_d2para of depth_prev_t
 * at the centre hypothesis' four corners), the glue workgroups write the log / memory features.  f_input [b,h,w,f_stride]:
 * channel order of m4d_level_front, padding channels untouched (the caller keeps them zero).  prev_l_parallax / prev_l_other
 * [b,ph,pw,1] / [b,ph,pw,4]: both NULL at the coarsest level.  Bit-identical to m4d_level_pre_normalize + m4d_dscv_sncv_fwd
 * (tests/test_gpu_ops.py::test_level_front_small_is_bitwise_the_separate_launches).  _supported: the pyramid's (C, cuts)
 * pairs, DSCV range 4 or 2. */
int m4d_level_front_small_supported(int C, int nbre_cuts, int dscv_range, int sncv_range);
int m4d_level_front_small(const float* norm_f, const float* prev_f, const float* depth_prev_t,
                          const float* prev_l_parallax, const float* prev_l_other, int ph, int pw,
                          const float* rot, int rot_c, const float* trans, const float* cam_f, const float* cam_c,
                          int b, int h, int w, int C, int nbre_cuts, int dscv_range, int sncv_range, int cv_accum,
                          float* f_input, int f_stride, float log_scale, void* stream);

/* The fused level front (m4depth_network.py:179-242 in one launch, default settings: all ablation blocks on, DSCV range 4,
 * SNCV range 3): per-cut normalisation of raw_f [b,h,w,C] -> norm_out (the buffer that becomes prev_f_maps, :211/:259);
 * x2 upsampling of the coarser level's parallax / other maps ([b,ph,pw,1] / [b,ph,pw,4]; both NULL at the coarsest level),
 * prev_d2para of depth_prev_t, DSCV against prev_f, SNCV of the normalised features, both log features -- assembled into
 * whole rows of f_input [b,h,w,f_stride] (channel order cv | log para_l | other(4) | sncv | log para_t, padding channels
 * zeroed), written as contiguous runs.  Bit-identical to m4d_level_pre_normalize + m4d_dscv_fwd + m4d_sncv_fwd.
 * m4d_level_front_supported: 1 if the (C, cuts, ranges, row stride) combination has a kernel (f_stride must be 58*cuts+6
 * rounded up to a multiple of 8), else 0 -- the caller then uses the three separate entry points. */
int m4d_level_front_supported(int C, int nbre_cuts, int dscv_range, int sncv_range, int f_stride);
int m4d_level_front(const float* raw_f, float* norm_out, const float* prev_f, const float* depth_prev_t,
                    const float* prev_l_parallax, const float* prev_l_other, int ph, int pw,
                    const float* rot, int rot_c, const float* trans, const float* cam_f, const float* cam_c,
                    int b, int h, int w, int C, int nbre_cuts, int cv_accum,
                    float* f_input, int f_stride, float log_scale, void* stream);
/* ... with the search ranges as arguments: (dscv_range, sncv_range) = (4, 3), the reference's hard-coded windows
 * (m4depth_network.py:221,232), or (6, 6), BASELINE configs[4] (13 hypotheses, 13x13 window: levels 1-5 of the 6-level pyramid;
 * f_stride = (2 dscv_range + 1 + (2 sncv_range + 1)^2) * cuts + 6 rounded up to a multiple of 8).  Bit-identical to the three
 * separate entry points with the same ranges. */
int m4d_level_front_r(const float* raw_f, float* norm_out, const float* prev_f, const float* depth_prev_t,
                      const float* prev_l_parallax, const float* prev_l_other, int ph, int pw,
                      const float* rot, int rot_c, const float* trans, const float* cam_f, const float* cam_c,
                      int b, int h, int w, int C, int nbre_cuts, int dscv_range, int sncv_range, int cv_accum,
                      float* f_input, int f_stride, float log_scale, void* stream);

/* Level-local intrinsics of DepthEstimatorPyramid.call (m4depth_network.py:300-302) for all levels in one launch:
 * f_out / c_out [levels,b,2], level l (0 = finest) = cam / 2^(l+1). */
int m4d_camera_pyramid(const float* cam_f, const float* cam_c, int b, int levels, float* f_out, float* c_out,
                       void* stream);

/* Fused "depth_estimator" tail of one level (:247-260): refiner_out [b,h,w,5] ->
 * parallax = exp(clip(out0,-7,7)) / scale, other = out[1:5], depth =
 * parallax2depth(parallax); depth is also stored into depth_state (may be NULL). */
int m4d_level_post(const float* refiner_out, const float* rot, int rot_c, const float* trans,
                   const float* cam_f, const float* cam_c, int b, int h, int w, float scale,
                   float* parallax, float* depth, float* other, float* depth_state, void* stream);

/* Convolution epilogue on an NHWC activation [rows, C] (rows = b*h*w): out = leaky_relu(x +
 * bias[c], slope) -- the bias add of Keras Conv2D and the tf.nn.leaky_relu(., 0.1) that
 * follows it (m4depth_network.py:84,87,123,133); slope = 1 gives the bias add alone (last
 * refiner convolution, :132).  In place when out == x. */
int m4d_bias_act(const float* x, const float* bias, long long rows, int C, float slope,
                 float* out, void* stream);

/* m4d_bias_act whose result lands inside a larger, zero-bordered [b,out_h,out_w,C] buffer at
 * (off_y,off_x): the TF 'SAME' padding of the stride-2 encoder convolution that consumes it
 * (m4depth_network.py:68-72; bottom/right only for even sizes) without a separate pad pass.
 * The caller keeps the border zero (the kernel never writes it).  C % 4 == 0. */
int m4d_bias_act_padded(const float* x, const float* bias, int b, int h, int w, int C, float slope,
                        float* out, int out_h, int out_w, int off_y, int off_x, void* stream);

/* Keras Conv2D(Cout, 3, strides 1, padding 'same') + bias + leaky_relu(slope) (slope = 1: no
 * activation) in one launch on the f32-input matrix cores (m4depth_network.py:104-135, :63-67).
 * x [b,h,w,Cin] NHWC (Cin even), out [b,h,w,Cout].  wp: the HWIO kernel re-packed by the host as
 * [ceil(Cin/16)][9 taps (ky*3+kx)][CoutPad][16] with CoutPad = Cout rounded up to 32, input
 * channels of a chunk stored even-first (0,2,..,14,1,3,..,15), zero padded
 * (m4depth_amd.network_ops.pack_conv_weights).  Deterministic; float32 exact (fmaf chain over
 * chunk, ky, kx, channel). */
int m4d_conv3x3_bias_act(const float* x, const float* wp, const float* bias, int b, int h, int w,
                         int Cin, int Cout, int CoutPad, float slope, float* out, void* stream);
/* Same, with a caller-owned workspace (m4d_conv3x3_workspace_floats floats) that lets small
 * problems (coarse pyramid levels: a handful of pixel tiles, K up to 9*470) split K over
 * workgroups; partial sums are reduced in split order by a second kernel (still deterministic). */
long long m4d_conv3x3_workspace_floats(int b, int h, int w, int CoutPad);
/* General form: stride 1 or 2 with TensorFlow 'SAME' padding computed inside (stride 2 on an even
 * size pads bottom/right only -- no padded copy of the input is needed); out is
 * [b, ceil(h/stride), ceil(w/stride), Cout].  Cin may be odd (the 3-channel input image). */
int m4d_conv3x3s_bias_act_ws(const float* x, const float* wp, const float* bias, int b, int h, int w,
                             int Cin, int Cout, int CoutPad, int stride, float slope, float* out,
                             float* workspace, long long workspace_floats, void* stream);
int m4d_conv3x3_bias_act_ws(const float* x, const float* wp, const float* bias, int b, int h, int w,
                            int Cin, int Cout, int CoutPad, float slope, float* out, float* workspace,
                            long long workspace_floats, void* stream);
/* m4d_conv3x3s_bias_act_ws with the split-K factor -- which sets the summation order -- decided for a launch on split_batch
 * images instead of this launch's b: the same layer launched on one frame or on several stacked frames of a batch-split_batch
 * sequence gives the same bits per image.  split_batch == b is m4d_conv3x3s_bias_act_ws. */
int m4d_conv3x3s_bias_act_wsb(const float* x, const float* wp, const float* bias, int b, int split_batch, int h, int w,
                              int Cin, int Cout, int CoutPad, int stride, float slope, float* out,
                              float* workspace, long long workspace_floats, void* stream);
/* Latency-first form of the same stride-1 layer for SMALL maps at batch 1 (round 5, csrc/m4d_convlat.hip; the DispRefiner
 * convolutions of the coarse pyramid levels, m4depth_network.py:116-135): every wave requests everything it needs -- its weight
 * fragments of at most two 16-channel chunks straight into MFMA operand registers, then the workgroup's halo -- in ONE memory
 * round trip; K is split over the waves of a workgroup (kw sub-slices, added in wave order) and over s_out workgroups, whose
 * raw partial tiles go to s_out slabs (out + z * out_slab_floats) that the CONSUMING call adds in slab order, + the producer's
 * bias and leaky_relu, while it stages its input (s_in / x_slab_floats / x_bias / x_slope; x_bias NULL = x is a finished
 * activation).  s_out == 1 writes the finished activation leaky_relu(sum + bias, slope).  float32 operands as exact 3 x bf16
 * splits (arithmetic of m4d_conv3x3_small6_bias_act; another summation order over K).  wp = network_ops.pack_conv_weights_lat
 * ([Cout/32][Cin/16][9 taps][3 parts][64 lanes][8] bf16: MFMA B-fragment order).  mt = 1 / 2 / 4 M-tiles (8x4 / 8x8 / 16x8
 * pixels per workgroup), kw = 1 / 2 / 4, 1 <= s_in <= 4, Cin >= 16, Cin % 4 == 0.  Deterministic. */
int m4d_conv3x3_lat(const float* x, int s_in, long long x_slab_floats, const float* x_bias, float x_slope,
                    const void* wp, const float* bias, int b, int h, int w, int Cin, int Cout, float slope,
                    int mt, int kw, int s_out, float* out, long long out_slab_floats, void* stream);
/* ... with stride 1 or 2 (TF 'SAME'; the coarse stride-2 layers of the encoder, m4depth_network.py:66-72): out / every slab
 * [b, ceil(h/stride), ceil(w/stride), Cout]. */
int m4d_conv3x3s_lat(const float* x, int s_in, long long x_slab_floats, const float* x_bias, float x_slope,
                     const void* wp, const float* bias, int b, int h, int w, int Cin, int Cout, int stride, float slope,
                     int mt, int kw, int s_out, float* out, long long out_slab_floats, void* stream);
/* m4d_conv3x3_lat with every float32 operand split into TWO fp16 terms after a power-of-two scale (per output pixel and wave
 * K range from the pixel's 3x3 window for the input, per output channel for the weights), three fp16 MFMA products per term
 * pair, float32 accumulation (csrc/m4d_convlat_f16.hip).  The slabs it writes and reads are m4d_conv3x3_lat's (raw, unscaled
 * float32 partial sums), so the two kernels chain either way.  wp = network_ops.pack_conv_weights_lat_f16:
 * [Cout/32][Cin/16][9 taps][2 parts][64 lanes][8] fp16 followed by [Cout/32 * 32] int16 weight exponents, 16-byte aligned.
 * Stride 1, mt = 1 / 2 / 4 (no M-over-waves form).  Deterministic.  Additive entry point: ABI 6 unchanged. */
int m4d_conv3x3_lat_f16(const float* x, int s_in, long long x_slab_floats, const float* x_bias, float x_slope,
                        const void* wp, const float* bias, int b, int h, int w, int Cin, int Cout, float slope,
                        int mt, int kw, int s_out, float* out, long long out_slab_floats, void* stream);
/* out = leaky_relu(bias + slab_0 + ... + slab_{s_in-1}, slope), slabs added in slab order: the finished form of a partial-sum
 * activation, for consumers that do not add the slabs themselves and for inspection.  C % 4 == 0. */
int m4d_partial_finish(const float* x, int s_in, long long x_slab_floats, const float* bias, float slope,
                       long long pixels, int C, float* out, void* stream);

/* The same stride-1 layer for SMALL maps (the DispRefiner convolutions of the coarsest pyramid levels, m4depth_network.py:
 * 116-135 at 6x20 ... 24x80 pixels): ONE launch -- a workgroup is an 8x4-pixel tile x 32 output channels whose four waves
 * walk interleaved 16-channel K chunks independently and add their partial tiles in wave order -- instead of the split-K
 * pair (partial sums + ordered reduce) the general entry needs there.  Cin >= 16, Cin % 4 == 0; same packed weights;
 * deterministic.  The caller picks it by map size (m4depth_amd.network: refiner layers with b*h*w <= 2048 and Cin <= 256). */
int m4d_conv3x3_small_bias_act(const float* x, const float* wp, const float* bias, int b, int h, int w,
                               int Cin, int Cout, int CoutPad, float slope, float* out, void* stream);
/* ... with stride 1 or 2 (the coarse stride-2 layers of the encoder): out [b, ceil(h/stride), ceil(w/stride), Cout]. */
int m4d_conv3x3s_small_bias_act(const float* x, const float* wp, const float* bias, int b, int h, int w,
                                int Cin, int Cout, int CoutPad, int stride, float slope, float* out, void* stream);
/* ... with float32 operands split exactly into three bf16 terms on the bf16 matrix cores (float32 accuracy, see
 * m4d_conv3x3_wino6_bias_act); wp6 = network_ops.pack_conv_weights_small6 ([Cin/16][9][CoutPad][3][16] bf16). */
int m4d_conv3x3_small6_bias_act(const float* x, const void* wp6, const float* bias, int b, int h, int w,
                                int Cin, int Cout, int CoutPad, float slope, float* out, void* stream);

/* DomainNormalization (m4depth_network.py:44-48) fused with the leaky_relu(slope) that follows it
 * at encoder level 0 (:82-84; slope = 1 for the normalisation alone).  x, out [b,h,w,C] (C = 16 or
 * 32); mean and the two-pass variance over (h,w) per (b,c); (x-mean)/(var+1e-12); l2-normalise
 * over channels; scale*n + bias.  workspace: m4d_dinl_workspace_floats(b, C) floats = b*512*C double partial sums, then
 * mean [b][C] and var [b][C] (floats) at its end. */
long long m4d_dinl_workspace_floats(int b, int C);
/* ... written into a [b,out_h,out_w,C] buffer at (off_y,off_x) (see m4d_bias_act_padded). */
int m4d_dinl_fwd_padded(const float* x, const float* scale, const float* bias, int b, int h, int w, int C,
                        float slope, float* workspace, float* out, int out_h, int out_w, int off_y,
                        int off_x, void* stream);
int m4d_dinl_fwd(const float* x, const float* scale, const float* bias, int b, int h, int w, int C,
                 float slope, float* workspace, float* out, void* stream);

/* Encoder level 0 (FeaturePyramid.call, m4depth_network.py:79-87 with DINL): the head of the network as two calls.
 * m4d_enc_head_fwd: conv3x3(images, w_hwio [3,3,3,16]) + bias -> raw_out [b,h,w,16], and the DINL statistics of
 *   raw_out into workspace (n = m4d_dinl_workspace_floats(b,16) floats): mean = the b*16 floats at n - 2*b*16, var the last b*16.
 *   Image n of the b = frames*bsz images starts at images + (n % bsz)*stride_b + (n / bsz)*stride_t floats: the frames of
 *   a [bsz,T,H,W,3] sequence batch (M4Depth.call encodes every frame, :358-360) are read in place, frame-major; a dense
 *   [b,h,w,3] batch is bsz = b, stride_b = h*w*3, stride_t = 0.
 * m4d_conv3x3s2_dinl_bias_act: the stride-2 convolution on leaky_relu(DomainNormalization(raw), dn_slope), the
 *   normalisation fused into its input staging; wp packed as for m4d_conv3x3s_bias_act_ws (CoutPad = 32). */
/* The same level in ONE call that never materialises the [b,h,w,16] map: conv3x3(3 -> 16) is recomputed from the images on
 * 16x16x4 MFMAs in each of three passes (channel sums, squared deviations, normalise + leaky_relu(dn_slope) + conv3x3
 * stride 2 (w2_hwio [3,3,16,16], TF 'SAME') + bias2 + leaky_relu(slope) -> out [b,(h+1)/2,(w+1)/2,16]).  Images addressed as
 * in m4d_enc_head_fwd; workspace m4d_dinl_workspace_floats(b,16) floats (mean / var left there as by m4d_enc_head_fwd). */
int m4d_enc_level0_fwd(const float* images, int bsz, long long stride_b, long long stride_t,
                       const float* w1_hwio, const float* bias1, const float* dn_scale, const float* dn_bias,
                       float dn_slope, const float* w2_hwio, const float* bias2, float slope,
                       int b, int h, int w, float* workspace, float* out, void* stream);
/* m4d_enc_level0_fwd as its two halves: the statistics passes (mean / var [b,16] of conv1's output per image and channel;
 * workspace >= m4d_dinl_workspace_floats(b,16) - 2*b*16 floats, 8-byte aligned: the double partial sums without the mean / var
 * tail) and the fused
 * normalise + stride-2 convolution pass reading them.  Per-image arithmetic: the statistics of all frames of a sequence may be
 * taken in one call and the frames applied in several (same bits as m4d_enc_level0_fwd on any grouping). */
int m4d_enc_level0_stats(const float* images, int bsz, long long stride_b, long long stride_t,
                         const float* w1_hwio, const float* bias1, int b, int h, int w, float* workspace,
                         float* mean, float* var, void* stream);
int m4d_enc_level0_apply(const float* images, int bsz, long long stride_b, long long stride_t,
                         const float* w1_hwio, const float* bias1, const float* mean, const float* var,
                         const float* dn_scale, const float* dn_bias, float dn_slope, const float* w2_hwio,
                         const float* bias2, float slope, int b, int h, int w, float* out, void* stream);
int m4d_enc_head_fwd(const float* images, int bsz, long long stride_b, long long stride_t,
                     const float* w_hwio, const float* bias, int b, int h, int w, int C,
                     float* workspace, float* raw_out, void* stream);
int m4d_conv3x3s2_dinl_bias_act(const float* x_raw, const float* mean, const float* var, const float* dn_scale,
                                const float* dn_bias, float dn_slope, const float* wp, const float* bias,
                                int b, int h, int w, int Cout, int CoutPad, float slope, float* out, void* stream);

/* The 7 metrics of metrics.py (AbsRel, SqRel, RMSE, RMSE_log, Delta1..3) of one batch in one
 * pass, including test_step's clipping gt in [0,max_d], est in [0.001,max_d]
 * (m4depth_network.py:465-467).  gt, est: n floats; out7: 7 floats (main.py:127-130 order);
 * workspace: m4d_metrics_workspace_bytes() bytes.  total7 (may be NULL): the 7 Keras-Mean totals, += out7 in the same
 * launch (compiled_metrics.update_state, :470); mean7 (may be NULL) = total7 / count, what test_step returns (:473-474). */
long long m4d_metrics_workspace_bytes(void);
int m4d_depth_metrics(const float* gt, const float* est, long long n, float max_d, void* workspace,
                      float* out7, float* total7, float count, float* mean7, void* stream);
/* The same with the ground truth read in place out of a larger tensor: image j (per_image floats) starts at
 * gt + j * gt_image_stride -- the last frame of a [b,T,H,W,1] sequence batch (test_step, m4depth_network.py:455-456) without
 * the dense copy a framework slice costs at batch > 1.  Same per-thread element order as the dense form: the same bits. */
int m4d_depth_metrics_strided(const float* gt, long long per_image, long long gt_image_stride, const float* est,
                              long long n, float max_d, void* workspace, float* out7, float* total7, float count,
                              float* mean7, void* stream);
/* The same 7 metrics for each sample of a batch on its own (batched streaming evaluation, main.py --eval_streams): gt, est are
 * [b][per_image] floats, sample s at gt + s * gt_stride / est + s * est_stride (strides >= per_image).  rows [b][7] floats:
 * row s is bit for bit what m4d_depth_metrics(gt_s, est_s, per_image, ...) writes to out7 (the same block partition, one
 * finalize workgroup per sample, the same fixed summation order; no atomics).  new_traj, active: uint8 [b] device masks;
 * counted [b] uint8 = active[s] && !new_traj[s] (read by the kernel only).  workspace:
 * m4d_metrics_per_sample_workspace_bytes(b) bytes (b x 512 x 9 doubles).  Additive entry point: ABI 6 unchanged. */
long long m4d_metrics_per_sample_workspace_bytes(int b);
int m4d_depth_metrics_per_sample(const float* gt, long long gt_stride, const float* est, long long est_stride, int b,
                                 long long per_image, float max_d, const unsigned char* new_traj, const unsigned char* active,
                                 void* workspace, float* rows, unsigned char* counted, void* stream);

/* ---- training without MIOpen (train_step, m4depth_network.py:371-399: tf.GradientTape through every Conv2D) ---------- */

/* Weight gradient of the 3x3 TF-'SAME' convolution y = conv(x [b,h,w,cin], W), stride 1 or 2, given g = dL/dy
 * [b,ceil(h/s),ceil(w/s),cout]: dw [cout][3][3][cin] floats (the memory layout of an OIHW parameter with channels-last
 * strides).  fp32 MFMA, two-stage fixed-order reduction over the pixels (deterministic).  cin < 8 is the 3-channel image
 * layer (stride 1, cout <= 32).  workspace: m4d_conv3x3_wgrad_workspace_floats(...) floats. */
long long m4d_conv3x3_wgrad_workspace_floats(int b, int h, int w, int cin, int cout, int stride);
int m4d_conv3x3_wgrad(const float* x, const float* g, int b, int h, int w, int cin, int cout, int stride,
                      float* workspace, long long workspace_floats, float* dw, void* stream);
/* g [b,ceil(h/2),ceil(w/2),C] spread onto the [b,h,w,C] grid of a stride-2 layer's input (zeros elsewhere), placed so that
 * the layer's data gradient is the stride-1 'SAME' convolution of the result with the rotated, transposed kernel
 * (m4d_pack_conv_weights(transpose = 1) + m4d_conv3x3s_bias_act_ws). */
int m4d_dilate2(const float* g, int b, int oh, int ow, int C, int h, int w, float* out, void* stream);

/* ---- dataloaders (midair / kitti / tartanair .py): _decode_samples after decompression ----------------------- */

/* RGB frames as the JPEG decoder leaves them, [n,ih,iw,3] uint8 -> [n,oh,ow,3] float32 =
 * tf.image.resize(cast(image)/255, [oh,ow]) (bilinear, half-pixel centres; midair.py:35-45,
 * kitti.py:25-36, tartanair.py:21-33). */
int m4d_decode_rgb8_resize(const uint8_t* images, int n, int ih, int iw, int oh, int ow, float* out,
                           void* stream);
/* Ground-truth maps [n,ih,iw] -> [n,oh,ow,1] float32.
 * kind 0  Mid-Air: uint16 bit patterns of float16 disparity, depth = 512/x, bilinear (midair.py:49-55)
 * kind 1  KITTI: uint16/256, nearest; crop (may be NULL) = {y0,y1,x0,x1} keeps [y0,y1)x[x0,x1) and
 *         zeroes the rest -- the Garg/Eigen evaluation mask (kitti.py:14-20,43-50)
 * kind 2  TartanAir: float32, nearest; rgb_resized (may be NULL) [n,oh,ow,3]: pixels whose colour
 *         is exactly black are zeroed (tartanair.py:37-45). */
int m4d_decode_depth_resize(const void* raw, int kind, int n, int ih, int iw, int oh, int ow,
                            const float* rgb_resized, const int crop[4], float* out, void* stream);

/* ---- a user's own recording (dataloaders/recording.py): lens undistortion fused into the decode ----------------- */

/* The undistortion table of one recording: for every pixel of the pinhole OUTPUT camera the index coordinates (u, v) of its
 * source in the distorted frame.  model 0 pinhole (dist may be NULL), 1 radtan (dist = k1 k2 p1 p2 k3: OpenCV / Kalibr),
 * 2 equidistant (dist = k1 k2 k3 k4: OpenCV fisheye / Kalibr).  dist, src_cam = {fx, fy, cx, cy} of the recording and
 * out_cam = {fx', fy', cx', cy'} of the output are HOST arrays (they travel to the kernel by value); principal points in the
 * half-pixel convention of get_coords_2d (pixel centres at integer + 0.5).  map [oh,ow,2] float32 in device memory.
 * Per output pixel (row, col), float32, one IEEE rounding per operation, in this order:
 *   x = (((float)col + 0.5f) - cx') / fx',  y = (((float)row + 0.5f) - cy') / fy'
 *   pinhole     : xd = x, yd = y
 *   radtan      : r2  = x*x + y*y
 *                 rad = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3))
 *                 xd  = x * rad + ((((2.0f * p1) * x) * y) + p2 * (r2 + (2.0f * x) * x))
 *                 yd  = y * rad + (p1 * (r2 + (2.0f * y) * y) + (((2.0f * p2) * x) * y))
 *   equidistant : r = sqrtf(x*x + y*y), th = atanf(r), th2 = th * th
 *                 thd = th * (1.0f + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4))))
 *                 s = r > 1e-8f ? thd / r : 1.0f;  xd = x * s, yd = y * s
 *   u = (xd * fx + cx) - 0.5f,  v = (yd * fy + cy) - 0.5f
 * The entry is (u, v) when -0.5f <= u <= (float)iw - 0.5f and -0.5f <= v <= (float)ih - 0.5f (inside the source image's pixel
 * area); otherwise, and for any non-finite value, it is (-1, -1): no source.  The pinhole and radtan tables are bit-exact
 * (+ - * / only, -ffp-contract=off); the equidistant one is as exact as the device's atanf.
 * Known limit: a radtan polynomial with strongly negative k1 folds over at large radius; output pixels beyond the fold (a
 * field of view widened far past the lens's) map back INTO the image and are not detected.
 * Returns 1 without a launch for: a model outside 0..2, a NULL src_cam, out_cam or map, a NULL dist for models 1 and 2, a
 * size <= 0, map off 8 bytes.  One plain launch (capturable).  Additive entry point: ABI 6 unchanged. */
int m4d_undistort_map(int model, const float* dist, const float src_cam[4], const float out_cam[4], int ih, int iw, int oh,
                      int ow, float* map, void* stream);
/* RGB frames as the decoder leaves them, [n,ih,iw,3] uint8, looked up through map [oh,ow,2] (one table for all n frames)
 * -> [n,oh,ow,3] float32.  Per output pixel, with (u, v) its entry:
 *   an entry with u < -0.5f or v < -0.5f (the table's (-1, -1)), a NaN or an infinity: 0, 0, 0
 *   otherwise, per axis as m4d_decode_rgb8_resize does from its source coordinate on: lo = clamp((int)floorf(u), 0, iw-1),
 *   hi = clamp((int)ceilf(u), 0, iw-1), lerp = u - floorf(u); every tap is (float)byte / 255.0f first;
 *   top = tl + (tr - tl) * xlerp, bot = bl + (br - bl) * xlerp, value = top + (bot - top) * ylerp.
 * With the table ((o + 0.5f) * scale - 0.5f) the result equals m4d_decode_rgb8_resize bit for bit.  Indices are clamped: no
 * table content reads outside the images (a finite coordinate past the image samples its border).  Returns 1 without a launch for: a NULL pointer, a size <= 0, map off 8 bytes,
 * out off 4.  One plain launch (capturable).  Additive entry point: ABI 6 unchanged. */
int m4d_decode_rgb8_remap(const uint8_t* images, const float* map, int n, int ih, int iw, int oh, int ow, float* out,
                          void* stream);
/* 16-bit depth maps registered to the colour camera, [n,ih,iw] uint16, through the same table -> [n,oh,ow,1] float32, nearest:
 *   column = clamp((int)floorf(u + 0.5f), 0, iw-1), row likewise;  out = (float)value * inv_scale
 * A source value of 0 (no measurement) and a no-source entry (as above: below -0.5, NaN or infinite) give exactly 0.  Returns 1 without a launch for: a NULL
 * pointer, a size <= 0, raw off 2 bytes, map off 8, out off 4.  One plain launch (capturable).  Additive entry point: ABI 6
 * unchanged. */
int m4d_decode_depth16_remap(const uint16_t* raw, const float* map, float inv_scale, int n, int ih, int iw, int oh, int ow,
                             float* out, void* stream);

/* ---- prediction export (main.py --mode=predict --save_dir): the mirror of the decoders above ------------------ */

/* The depth estimate of a frame batch -> what goes to disk, in one launch.  est [b,h,w,1], gt [b,h,w,1] (may be NULL),
 * rgb [b,h,w,3] in 0..1 (may be NULL): float32, image i at ptr + i * stride ELEMENTS (est_stride, gt_stride >= h*w,
 * rgb_stride >= 3*h*w: views of larger buffers are read in place); est is read once per pixel.  Outputs are dense:
 *   depth16 [b,h,w] uint16, format 0 none (depth16 may be NULL), 1 kitti16, 2 midair16 -- the encodings kind 1 / kind 0 of
 *           m4d_decode_depth_resize read back;
 *   panels  [b, n_panels*h, w, 3] uint8: n_panels (0..4) RGB8 images stacked vertically in the order of panel_kinds (a HOST
 *           array): 0 rgb, 1 est, 2 gt, 3 err;  lut [257,3] uint8 in device memory, row 256 = the colour of invalid pixels
 *           (needed by kinds 1..3; gt by 2, 3; rgb by 0).
 * float32, one IEEE rounding per operation, in this order (rintf = round half to even):
 *   valid(d)  = isfinite(d) && d > 0
 *   kitti16   : valid -> (uint16) min(max(rintf(d * 256.0f), 1.0f), 65535.0f), else 0
 *   midair16  : valid -> bits of half_rne(512.0f / d), else 0x7C00 (an overflowing quotient is 0x7C00 as well; the Mid-Air
 *               decoder reads 0x7C00 as depth 0)
 *   est / gt  : valid -> lut[(int) rintf(min(max((1.0f/d - 1.0f/far) / (1.0f/near - 1.0f/far), 0.0f), 1.0f) * 255.0f)],
 *               else lut[256] -- inverse depth, linear between far and near
 *   err       : est and gt valid -> lut[(int) rintf(min((fabsf(est - gt) / gt) / err_max, 1.0f) * 255.0f)], else lut[256]
 *   rgb       : (uint8) rintf(min(max(v, 0.0f), 1.0f) * 255.0f), NaN -> 0
 * Returns 1 without a launch for: a NULL est, format outside 0..2, depth16 missing for a format, nothing asked for, more
 * than 4 panels or an unknown kind, gt / rgb / lut / panels missing for a panel that needs them, near <= 0, far <= near,
 * err_max <= 0, a stride smaller than an image, float pointers off 4 bytes or depth16 off 2.  Every output element is
 * written; plain launch (capturable).  Additive entry point: ABI 6 unchanged. */
int m4d_depth_export(const float* est, long long est_stride, const float* gt, long long gt_stride, const float* rgb,
                     long long rgb_stride, int b, int h, int w, int format, uint16_t* depth16, int n_panels,
                     const int* panel_kinds, const uint8_t* lut, float near, float far, float err_max, uint8_t* panels,
                     void* stream);

/* ---- point clouds (main.py --mode=predict --save_dir --save_cloud): the estimate as 3-D geometry ------------------------ */

/* One camera-to-world pose per sample, kept on the device (the host never reads it): pose [b,7] float64 = qw qx qy qz tx ty tz,
 * in / out.  rot [b,4] quaternion w,x,y,z, trans [b,3]: the frame-to-frame motion the network gets, in the convention
 * reproject implies (utils/depth_operations.py:72-105): a point X of the current camera is R(rot) X + trans in the previous
 * camera.  The world is the camera of the trajectory's first frame.  reset [b] uint8 device mask (may be NULL = nobody).
 *   force_all || reset[s] : pose[s] = (1,0,0,0; 0,0,0); rot / trans of that sample are not read
 *   otherwise             : q = rot[s] / |rot[s]|            (float64; |.| = sqrt(((w*w + x*x) + y*y) + z*z))
 *                           tw <- R(qw_old) trans[s] + tw_old  (R as get_rot_mat writes it, in float64, rows summed left to right)
 *                           qw <- (qw_old q) / |qw_old q|      (Hamilton product: R(qw) = R(qw_old) R(q))
 * All of it float64, one rounding per operation.  Unlike get_rot_mat (utils/depth_operations.py:18-53), which uses the
 * quaternion as it comes, both the incoming quaternion and the product are renormalised: the network sees one float32
 * quaternion per frame, this state is the product of thousands of them, and without the renormalisation its norm drifts and
 * R(qw) stops being a rotation (the cloud shears and scales).  Only rot_c = 4: a small-angle rot has no exact composition.
 * A zero or non-finite quaternion makes the sample's pose NaN until its next reset.
 * Returns 1 without a launch for: a NULL rot, trans or pose, b <= 0, rot / trans off 4 bytes, pose off 8.  One plain launch
 * (capturable).  Additive entry point: ABI 6 unchanged. */
int m4d_pose_accumulate(const unsigned char* reset, int force_all, const float* rot, const float* trans, int b, double* pose,
                        void* stream);

/* The depth maps of one step -> dense lists of coloured vertices.  depth [b,h,w,1], rgb [b,h,w,3] in 0..1: float32, image i at
 * ptr + i * stride ELEMENTS (depth_stride >= h*w, rgb_stride >= 3*h*w: views are read in place); cam_f, cam_c [b,2];
 * pose [b,7] float64 as m4d_pose_accumulate keeps it, or NULL = camera frame.
 * A pixel (row, col) is kept when row % step == 0, col % step == 0, its depth d is finite and near <= d <= far.  Its vertex is
 * 16 bytes: float32 x, y, z, then uint8 r, g, b, a:
 *   x = (((col + 0.5f) - cx) / fx) * d,  y = (((row + 0.5f) - cy) / fy) * d,  z = d     (float32, get_coords_2d's operand order)
 *   with pose: (x, y, z) <- (float) (R(q) (x, y, z) + t), R as get_rot_mat writes it and every operation in float64, rows
 *              summed left to right, then t added: one rounding to float32 at the end
 *   r, g, b = m4d_depth_export's rgb rule: (uint8) rintf(min(max(v, 0.0f), 1.0f) * 255.0f), NaN -> 0;  a = 255
 * vertices [b, cap, 16 bytes] with cap = ceil(h/step) * ceil(w/step): the kept vertices of sample s are written densely from
 * vertices[s][0] in raster order (deterministic: comparable byte for byte), one 16-byte store each; counts[s] int32 = their
 * number; the tail beyond the count is left untouched.  workspace: m4d_depth_cloud_workspace_ints(b,h,w,step) int32.
 * Two plain launches (capturable): a per-workgroup count, then the write pass, in which a workgroup sums the counts of the
 * workgroups before it in its sample and places its vertices by wave64 ballots; no workgroup waits on another, no atomics.
 * The write pass reads one count per earlier workgroup of the sample, so its cost grows with cap squared: cap > 2^24 (4096 x
 * 4096 candidates) is refused.
 * Returns 1 without a launch for: a NULL depth, rgb, cam_f, cam_c, vertices, counts or workspace, b <= 0 or > 65535, h or
 * w <= 0, step < 1, cap > 2^24, far <= near (or a NaN bound), a stride smaller than an image, float / int pointers off 4 bytes, pose off
 * 8, vertices off 16.  Additive entry points: ABI 6 unchanged. */
int m4d_depth_cloud(const float* depth, long long depth_stride, const float* rgb, long long rgb_stride, const float* cam_f,
                    const float* cam_c, const double* pose, int b, int h, int w, int step, float near, float far,
                    void* vertices, int* counts, int* workspace, void* stream);
/* int32 elements of m4d_depth_cloud's workspace (0 for a geometry it refuses). */
long long m4d_depth_cloud_workspace_ints(int b, int h, int w, int step);

/* ---- Multi-view depth check (main.py --save_cloud --cloud_views K): keep a pixel only if earlier frames confirm it (csrc/m4d_confidence.hip) ---- */

/* The forward-backward reprojection check of multi-view stereo fusion (MVSNet, Yao et al. ECCV 2018; COLMAP's fusion), against
 * up to K = views earlier frames of the sample's own trajectory, kept in a ring on the device.
 * depth [b,h,w,1] float32, image s at depth + s * depth_stride ELEMENTS (>= h*w: read in place); cam_f, cam_c [b,2]: the
 * sample's full-resolution camera, assumed the same for every frame since the sample's last reset; pose [b,7] float64 camera-to-
 * world as m4d_pose_accumulate leaves it (qw qx qy qz tx ty tz), used as stored (not renormalised); reset [b] uint8 device mask
 * (may be NULL = nobody).
 * State: ring_depth [(K+1),b,h,w] float32 and ring_pose [(K+1),b,7] float64.  Slot `head` (0..K) is WRITTEN by this call; the
 * slots (head - j) mod (K+1), j = 1..K, hold the frames j steps back and are only read, so the slot written is never one that
 * is read and the launch needs no ordering between workgroups.  The host advances head by one mod K+1 after every call.
 * age_in / age_out [b] int32, distinct buffers the host swaps after every call: the earlier frames of the sample's trajectory
 * the ring holds.
 *   a = (force_all || reset[s]) ? 0 : min(age_in[s], K)      (a negative age_in counts as 0)
 *   age_out[s] = min(a + 1, K)
 * Only the views j = 1..a are looked at: after a reset the other slots may hold another trajectory, or nothing.
 * Per pixel (row, col) of sample s, d = depth as it comes:
 *   d not finite or d <= 0 : n_views = 0.  Otherwise, float32 with m4d_depth_cloud's operand order:
 *   Xc = ((((col + 0.5f) - cx) / fx) * d, (((row + 0.5f) - cy) / fy) * d, d)
 *   and from here float64, one rounding per operation; f and c are the float32 values widened.  R(q) as get_rot_mat writes it.
 *   View j, (qk, tk) = ring_pose of its slot, (qc, tc) = pose[s]:
 *     Rr = R(qk)^T R(qc):  Rr[i][j] = (Rk[0][i] Rc[0][j] + Rk[1][i] Rc[1][j]) + Rk[2][i] Rc[2][j]
 *     tr = R(qk)^T (tc - tk): D = tc - tk;  tr[i] = (Rk[0][i] D[0] + Rk[1][i] D[1]) + Rk[2][i] D[2]
 *     X  = Rr Xc + tr:      X[i] = ((Rr[i][0] Xc.x + Rr[i][1] Xc.y) + Rr[i][2] Xc.z) + tr[i];   z = X[2]
 *     u  = ((fx X[0]) / z + cx) - 0.5,  v = ((fy X[1]) / z + cy) - 0.5        (integer values are pixel centres)
 *     the view TESTS the pixel when z > 0, 0 <= u <= w-1, 0 <= v <= h-1 and the four taps below are finite and > 0:
 *       u32 = (float) u, x0 = min((int) floorf(u32), w-2), ax = u32 - (float) x0;  v32, y0, ay likewise (indices are clamped to
 *       the map before any load);  d00, d01, d10, d11 = ring_depth[slot][s] at (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1);
 *       float32: top = d00 + ax * (d01 - d00), bot = d10 + ax * (d11 - d10), dk = top + ay * (bot - top)
 *     back:  Yk = ((((u + 0.5) - cx) / fx) * dk, (((v + 0.5) - cy) / fy) * dk, dk);  E = Yk - tr;
 *            Yc = Rr^T E:   Yc[i] = (Rr[0][i] E[0] + Rr[1][i] E[1]) + Rr[2][i] E[2];  Yc[2] > 0 is required
 *            pu = ((fx Yc[0]) / Yc[2] + cx) - 0.5,  pv = ((fy Yc[1]) / Yc[2] + cy) - 0.5
 *     the view CONFIRMS the pixel when  (pu - col)^2 + (pv - row)^2 < (double) tol_px * (double) tol_px  and
 *            fabs(Yc[2] - d) < (double) tol_rel * d          (no square root, no division)
 *   n_views [b,h,w] uint8 = the number of confirming views, 0..a;
 *   depth_f [b,h,w] float32 (may be NULL) = the bits of d where n_views >= min_views, else the quiet NaN 0x7FC00000;
 *   ring_depth[head][s] = the bits of d, unfiltered; ring_pose[head][s] = pose[s].
 * A NaN pose (a zero quaternion upstream) makes every comparison false: n_views = 0.  Every element of n_views, depth_f, the ring
 * slot `head` and age_out is written and nothing else; no atomics, no zero-fill; sample s of a batch launch equals a launch on
 * sample s alone bit for bit.  One plain launch: capturable for fixed arguments, but head and the age buffers change per frame,
 * so export.PredictionWriter calls it eagerly.  Four pixels per thread; when h*w and depth_stride are multiples of 4, depth,
 * ring_depth and depth_f 16-byte and n_views 4-byte aligned, they leave as one dword and 16-byte stores, else element by element
 * with the same bits.
 * Returns 1 without a launch for: a NULL pointer other than reset or depth_f, b outside 1..65535, h or w < 2, h*w > 2^24, views
 * outside 1..8, head outside 0..views, min_views outside 1..views, tol_px or tol_rel not > 0 (NaN included), age_in == age_out,
 * depth_stride < h*w, a float / int pointer off 4 bytes, pose or ring_pose off 8.  Additive entry points: ABI 6 unchanged. */
int m4d_depth_views(const float* depth, long long depth_stride, const float* cam_f, const float* cam_c, const double* pose,
                    const unsigned char* reset, int force_all, int b, int h, int w, int views, int head, float* ring_depth,
                    double* ring_pose, const int* age_in, int* age_out, float tol_px, float tol_rel, int min_views,
                    unsigned char* n_views, float* depth_f, void* stream);
/* float32 elements of m4d_depth_views' ring_depth, (views+1) b h w; -1 for a geometry it refuses. */
long long m4d_depth_views_ring_floats(int b, int h, int w, int views);

/* ---- Voxel maps (main.py --save_dir --save_map VOXEL): the clouds of a trajectory merged into one map (csrc/m4d_voxelmap.hip) ---- */

/* The map of a trajectory is the voxel-grid reduction of the vertices of that trajectory's per-frame clouds: its input is exactly
 * the 16-byte vertices m4d_depth_cloud wrote for those frames (float32 x, y, z in the world frame, uint8 r, g, b, a; whatever
 * stride, depth range and multi-view filter made them) and nothing is recomputed from depth.  Every accumulator is an unsigned
 * 64-bit integer, so the map does not depend on the order in which threads arrive and can be compared bit for bit.
 *
 * Per vertex, voxel = the float32 edge length widened to double:
 *   a non-finite x, y or z                                            : dropped_range += 1
 *   gx = (double) x / voxel,  ix = floor(gx);  ix < -2^20 or >= 2^20  : dropped_range += 1        (likewise y, z)
 *   ox = min((int) floor((gx - ix) * 256.0), 255)      in 0..255 (the minimum only acts where gx - ix rounds to 1.0: a negative
 *                                                      gx closer to zero than 2^-54)
 *   key = ((ix + 2^20) << 42) | ((iy + 2^20) << 21) | (iz + 2^20);   the empty slot is all ones, which no key is
 *   the voxel's record: n += 1, sx += ox, sy += oy, sz += oz, sr += r, sg += g, sb += b;
 *   old = atomic max(last_stamp, stamp);  old < stamp : frames += 1     -- exactly one arrival per voxel and call sees that, so
 *   frames is the number of distinct stamps (frames) that observed the voxel, whatever the order.
 *
 * State: one buffer of m4d_voxel_map_state_words(b, L) unsigned 64-bit words, 8-byte aligned:
 *   words [4 s, 4 s + 4)                     : the statistics of sample s -- observations (vertices read), dropped_range,
 *                                              dropped_full, occupied (slots claimed);
 *   words 4 b + (s 2^L + slot) 10 + 0 .. 9   : the record of `slot` of sample s -- key, n, sx, sy, sz, sr, sg, sb, last_stamp,
 *                                              frames.  An empty record is key = all ones and nine zeros.
 * The table of a sample is an open-addressing table of 2^L slots, L in 6..26, with linear probing from the top L bits of
 * key * 0x9E3779B97F4A7C15 (mod 2^64); 80 bytes per slot: 168 MB per sample at L = 21.  A key lives in one slot only; which one
 * depends on the arrival order, the record's content does not.
 *
 * m4d_voxel_map_integrate: vertices [b, cap, 16 bytes] and counts [b] int32 as m4d_depth_cloud left them on the device (a count
 * is clamped to 0..cap); stamp >= 1, the same for the whole call.  One launch, one thread per vertex.  Keys are read and claimed
 * with agent-scope atomics only (a load, a compare-and-swap), the sums are agent-scope atomic adds.  The probe of a vertex takes
 * at most 128 trips; a vertex whose probe runs out, or that meets an empty slot while `occupied` has reached 3/4 of the slots, is
 * counted in dropped_full and stored nowhere (claims already on their way when the mark is reached still land: occupied may pass
 * the mark by the number of those).  Nothing waits for another thread and no loop depends on what the table holds.  Lanes of a
 * wave that follow each other with one key are summed in registers first and their first lane issues the atomics: integer sums,
 * the same bits.  observations = n summed over the table + dropped_range + dropped_full, always.
 * A batch launch leaves in the table of sample s what a launch on sample s alone leaves; a sample with counts[s] = 0 is not
 * touched.
 *
 * m4d_voxel_map_extract: the records of sample s with frames >= min_frames, compacted in no particular order:
 *   keys_out[i] = key (unsigned 64-bit),  vertices_out[i] = 16 bytes like a cloud vertex:
 *   px = (float) (((double) ix + ((double) sx / (double) n + 0.5) / 256.0) * voxel)        (likewise y, z)
 *   r = (2 sr + n) / (2 n) in integer arithmetic (the mean rounded half up; likewise g, b),  a = min(frames, 255).
 *   count: one unsigned 64-bit device word the caller zeroes; the launch adds the number of qualifying records to it.  Records
 *   beyond out_cap are counted and not written.  One launch; the state is only read.
 *
 * m4d_voxel_map_clear: one launch that makes every record of the samples with mask[s] != 0 (mask NULL: of all samples) empty and
 * their statistics zero.  A fresh state is a cleared one.
 *
 * Each returns 1 without a launch for: a NULL pointer (other than mask), b outside 1..65535, L outside 6..26, cap outside
 * 1..2^24, voxel not > 0 or not finite, stamp < 1, s outside 0..b-1, min_frames < 1, out_cap < 1, state / keys_out / count off 8
 * bytes, vertices / vertices_out off 16, counts off 4.  Plain launches (capturable).  Additive entry points: ABI 6 unchanged. */
int m4d_voxel_map_integrate(const void* vertices, const int* counts, int b, int cap, float voxel, long long stamp, void* state,
                            int log2_slots, void* stream);
int m4d_voxel_map_extract(const void* state, int b, int log2_slots, int s, int min_frames, float voxel, void* keys_out,
                          void* vertices_out, long long out_cap, void* count, void* stream);
int m4d_voxel_map_clear(void* state, const unsigned char* mask, int b, int log2_slots, void* stream);
/* unsigned 64-bit words of the state, b (4 + 10 * 2^L); -1 for a geometry the entries refuse. */
long long m4d_voxel_map_state_words(int b, int log2_slots);

/* ---- TSDF surface meshes (main.py --save_dir --save_mesh VOXEL): one triangle mesh per trajectory (csrc/m4d_tsdf.hip) ---- */

/* Truncated-signed-distance fusion (Curless & Levoy 1996, KinectFusion) on a hashed voxel grid (Niessner et al. 2013) of the
 * depth maps of a trajectory, and a naive-surface-nets extraction: one vertex per sign-changing cell, one quad per sign-changing
 * grid edge.  Inputs as m4d_depth_cloud takes them: depth [b,h,w,1] / rgb [b,h,w,3] float32 at a batch stride in ELEMENTS,
 * cam_f, cam_c [b,2], pose [b,7] float64 camera-to-world (qw qx qy qz tx ty tz, used as stored; required).  voxel = the float32
 * edge length widened to double, K = trunc (2..8), T = (float) ((double) K * voxel) the truncation distance.  R = R(q) as
 * get_rot_mat writes it, in float64 (m4d_depth_cloud's expressions).  One IEEE rounding per operation throughout.
 *
 * State: one buffer of m4d_tsdf_state_words(b, L) unsigned 64-bit words, 8-byte aligned, structure of arrays:
 *   words [4 s, 4 s + 4)                        : the statistics of sample s -- occupied, dropped_range, dropped_full, updates;
 *   words 4 b + s 2^L + slot                    : keys[s][slot], the voxel map's key ((ix + 2^20) << 42) | ((iy + 2^20) << 21) |
 *                                                 (iz + 2^20); the empty slot is all ones;
 *   bytes 8 (4 b + b 2^L) + 24 (s 2^L + slot)   : recs[s][slot] -- float32 S (the sum of the truncated signed distances in units
 *                                                 of T), then uint32 n, sr, sg, sb, nc.  An empty record is all zero.
 * 32 bytes per slot: 134 MB per sample at L = 22.  The table is the voxel map's: linear probing from the top L bits of
 * key * 0x9E3779B97F4A7C15, at most 128 trips, no empty slot claimed once `occupied` has reached 3/4 of the slots.
 * A sample whose pose holds a non-finite number is skipped by both per-frame launches: nothing of it is read or written.
 *
 * m4d_tsdf_allocate: one launch, one thread per pixel (every pixel: no stride).  A pixel with d finite and near <= d <= far:
 *   ax = ((col + 0.5f) - cx) / fx,  ay = ((row + 0.5f) - cy) / fy                      (float32, then widened)
 *   for k = -2K .. 2K:  z = (double) d + (double) k * (voxel * 0.5);  only z > 0;   X = ax * z, Y = ay * z
 *     Pw[i] = ((R[i][0] X + R[i][1] Y) + R[i][2] z) + t[i];   cell[i] = floor(Pw[i] / voxel)
 *     a cell outside [-2^20, 2^20) (or not finite): dropped_range += 1.  Otherwise the key is claimed: agent-scope load and
 *     compare-and-swap; a claim writes the key only and adds 1 to occupied.  A sample whose probe runs out, or that meets an
 *     empty slot at the 3/4 mark, adds 1 to dropped_full (only "zero or not" is contract for that counter).
 *   A thread does not probe again for the key it has just found (consecutive samples of a ray share voxels): the SET of keys is
 *   the same, and it is the same for every schedule while the table stays below the mark.
 *
 * m4d_tsdf_integrate: one launch after allocate, every slot of every sample has one thread; a record is touched by its owner only, so S does
 *   not depend on the schedule.  Per non-empty slot with cell i:
 *   D[j] = ((double) i[j] + 0.5) * voxel - t[j];   X[j] = (R[0][j] D[0] + R[1][j] D[1]) + R[2][j] D[2];   z = X[2] > 0 required
 *   u = (fx X[0]) / z + cx,  v = (fy X[1]) / z + cy   (f, c widened);  0 <= u < w and 0 <= v < h required (false for NaN)
 *   d = depth[(int) floor(v)][(int) floor(u)], finite and near <= d <= far required;   sdf = (float) ((double) d - z)
 *   sdf < -T: nothing.  Otherwise S = S + fminf(sdf, T) / T, n += 1, and when sdf <= T also sr, sg, sb += the pixel's colour
 *   under m4d_depth_export's rgb rule and nc += 1.  updates += the records updated (one atomic add per workgroup, which walks its slots in a loop).
 *
 * m4d_tsdf_extract_vertices: sample s, one thread per slot; the state is only read.  The slot's voxel k is the min corner of the
 *   cell whose corners are the voxel centres k + {0,1}^3, corner c = dx | dy << 1 | dz << 2.  The cell is valid when all eight
 *   exist (read-only probe, the insertion's sequence, ending at an empty slot) with n >= min_frames.  D_c = S / (float) n;
 *   inside = D_c < 0.  A valid cell with both signs emits (key, 16-byte vertex):
 *   edges in the order axis x, y, z and, within axis a, the corners c without bit a ascending, edge (c, c | 1 << a); for every
 *   edge with inside(c) != inside(c | 1 << a):  t = D_a / (D_a - D_b);  sum[a] += t,  sum[j != a] += (float) bit j of c;
 *   local[j] = sum[j] / (float) edges;   p[j] = (float) ((((double) i[j] + 0.5) + (double) local[j]) * voxel)     (float32 sums)
 *   r = (2 SUM sr + SUM nc) / (2 SUM nc) over the eight corners in integer arithmetic (0 when SUM nc = 0; likewise g, b),
 *   a = min(255, min n).  count: one unsigned 64-bit device word the caller zeroes; records beyond out_cap are counted only.
 *
 * m4d_tsdf_extract_faces: the same launch shape.  Per voxel k with n >= min_frames and axis a (0 x, 1 y, 2 z; b = (a+1) % 3,
 *   c = (a+2) % 3): when k + e_a exists with n >= min_frames and inside(k) != inside(k + e_a), one quad of five 64-bit words:
 *   word 0 = a | (inside(k) ? 0 : 4);  words 1..4 = the cell keys k, k - e_b, k - e_b - e_c, k - e_c when inside(k), and in
 *   the reverse order otherwise (the owner key k is word 1 or word 4; the face's normal points from inside to outside).
 *   Nothing is emitted when k[a] is the largest index or k[b] or k[c] the smallest.  Whether the four cells have vertices is
 *   the host's business.  count / out_cap (in quads) as above.
 *
 * m4d_tsdf_clear: one launch; the samples with mask[s] != 0 (mask NULL: all) get empty keys, zero records and zero statistics.
 *
 * Each returns 1 without a launch for: a NULL pointer (other than mask), b outside 1..65535, L outside 6..26, h or w < 1,
 * h*w > 2^24, far <= near (NaN included), voxel not > 0 or not finite, trunc outside 2..8, a stride smaller than an image, s
 * outside 0..b-1, min_frames < 1, out_cap < 1, a float pointer off 4 bytes, pose / state / keys_out / quads_out / count off 8,
 * vertices_out off 16.  Plain launches (capturable).  Additive entry points: ABI 6 unchanged. */
int m4d_tsdf_allocate(const float* depth, long long depth_stride, const float* cam_f, const float* cam_c, const double* pose,
                      int b, int h, int w, float near, float far, float voxel, int trunc, void* state, int log2_slots,
                      void* stream);
int m4d_tsdf_integrate(const float* depth, long long depth_stride, const float* rgb, long long rgb_stride, const float* cam_f,
                       const float* cam_c, const double* pose, int b, int h, int w, float near, float far, float voxel, int trunc,
                       void* state, int log2_slots, void* stream);
int m4d_tsdf_extract_vertices(const void* state, int b, int log2_slots, int s, int min_frames, float voxel, void* keys_out,
                              void* vertices_out, long long out_cap, void* count, void* stream);
int m4d_tsdf_extract_faces(const void* state, int b, int log2_slots, int s, int min_frames, void* quads_out, long long out_cap,
                           void* count, void* stream);
int m4d_tsdf_clear(void* state, const unsigned char* mask, int b, int log2_slots, void* stream);
/* unsigned 64-bit words of the state, b (4 + 4 * 2^L); -1 for a geometry the entries refuse. */
long long m4d_tsdf_state_words(int b, int log2_slots);

/* ---- fused depth per frame (main.py --fused VOXEL, --save_fused): the TSDF volume rendered into a camera (csrc/m4d_tsdf.hip) ---- */

/* m4d_tsdf_raycast: the second half of KinectFusion -- every pixel's ray is marched through the field of the state above and
 * the z-depth (the network's convention) of the first front-face zero crossing is written.  One launch, one thread per pixel; the
 * state is only read: the launch runs after m4d_tsdf_integrate on the same stream.  state / b / log2_slots, cam_f, cam_c [b,2],
 * pose [b,7] float64, voxel, K = trunc as above; depth_out [b,h,w,1] float32, guide and fill likewise (or NULL), each at its
 * batch stride in ELEMENTS.  One IEEE rounding per operation, float64 where m4d_tsdf_allocate uses it and in its operand order,
 * so that the two agree on the voxel a point falls in.
 *   Per sample s: a pose that holds a non-finite number makes every pixel a miss.  R = R(q), t = pose[4..6]; voxel widened to
 *   double, hv = voxel * 0.5.
 *   Per pixel (row, col): ax = ((col + 0.5f) - cx) / fx,  ay = ((row + 0.5f) - cy) / fy             (float32, then widened)
 *   March range: z_lo = (double) near, z_hi = (double) far.  With guide != NULL and g = guide[s * guide_stride + px] finite,
 *   near <= g <= far:  Wd = ((double) window * (double) K) * voxel,  z_lo = fmax(near, (double) g - Wd),
 *   z_hi = fmin(far, (double) g + Wd); any other guide pixel marches the whole range.
 *   Positions: z_i = z_lo + (double) i * hv for i = 0 .. n_max = (long long) floor((z_hi - z_lo) / hv).
 *   Sample i: X = ax * z_i, Y = ay * z_i;  Pw[j] = ((R[j][0] X + R[j][1] Y) + R[j][2] z_i) + t[j];  cell[j] = floor(Pw[j] / voxel).
 *     KNOWN when the three cells lie in [-2^20, 2^20), the key is found (read-only probe, the insertion's sequence, ending at
 *     an empty slot) and its record has n >= min_frames and n > 0; then D = S / (float) n.  UNKNOWN otherwise.
 *   March, state (i, mode, run, prev), from i = 0, coarse, no prev, while i <= n_max:
 *     coarse, unknown: i += 2K (one truncation distance in z).
 *     coarse, known  : i = (i == 0 ? 0 : i - 2K + 1), the position just after the last unknown coarse one; mode = fine, run = 0,
 *                      no prev; position i is sampled again.
 *     fine, unknown  : no prev, run += 1; when run == 2K: mode = coarse, i += 2K; else i += 1.
 *     fine, known    : run = 0.  With a prev (of position i - 1), prev >= 0 and D < 0: the HIT,
 *                      z* = z_{i-1} + hv * (double) (prev / (prev - D))      (the quotient float32, then widened).
 *                      Otherwise prev = D, i += 1.
 *   The first positive-to-negative crossing between two consecutive known samples wins; negative-to-positive crossings (back
 *   faces) and crossings across an unknown sample are none.  After a back-up the fine walk reaches the known coarse position
 *   before run can reach 2K, so a position is sampled at most once per mode: 2 (n_max + 1) trips at most.
 *   Output: depth_out[s * out_stride + px] = (float) z* on a hit; on a miss fill[s * fill_stride + px] when fill != NULL, else
 *   the quiet NaN 0x7FC00000.  depth_out may be fill itself when the two strides are equal (a pixel is read before it is written,
 *   by its own thread); any other overlap of depth_out with fill or guide is undefined.
 *   hits: NULL, or b unsigned 64-bit words; the launch ADDS the hits of sample s to hits[s] (one integer atomic add per
 *   workgroup: the value is order-free).  The caller zeroes the words.
 * A thread does not probe for a key that the previous sample of its ray had; a wave is an 8x8 pixel tile.  Neither changes a bit.
 * Returns 1 without a launch for: a NULL state, cam_f, cam_c, pose or depth_out, b outside 1..65535, L outside 6..26, h or
 * w < 1, h*w > 2^24, far <= near or near <= 0 (NaN included), voxel not > 0 or not finite, trunc outside 2..8, min_frames < 1,
 * window < 1 with a guide, ((double) far - (double) near) / ((double) voxel * 0.5) > 2^20 (the march's constant bound), a stride
 * smaller than an image, a float pointer off 4 bytes, state / pose / hits off 8.  Plain launch (capturable).  Additive entry
 * point: ABI 6 unchanged. */
int m4d_tsdf_raycast(const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c, const double* pose,
                     int h, int w, float near, float far, float voxel, int trunc, int min_frames,
                     const float* guide, long long guide_stride, int window,
                     const float* fill, long long fill_stride,
                     float* depth_out, long long out_stride, void* hits, void* stream);

/* m4d_tsdf_render: m4d_tsdf_raycast with a choice of how the field is sampled and, per pixel, the normal and the colour of the
 * surface it hit.  The arguments of m4d_tsdf_raycast, interp (0 nearest voxel, 1 trilinear) and three optional outputs, each NULL
 * or at a batch stride of its own in ELEMENTS: normal_out [b,h,w,3] float32 (unit, camera frame), colour_out [b,h,w,3] float32 in
 * [0,1], view_out [b,h,w,3] uint8 (a shaded RGB8 picture).  depth_out is required.  One launch, one thread per pixel, a wave an 8x8
 * pixel tile, the state only read.  One IEEE rounding per operation; lerp(a, b, t) = a + t * (b - a) in float32 (a subtraction, a
 * product, a sum).  Corner c = dx | dy << 1 | dz << 2 of a base cell B is the voxel B + (dx, dy, dz).
 *   Positions, Pw, cell, KNOWN, the march and its state are m4d_tsdf_raycast's: unknown space is visited exactly as there.
 *   Base cell and fractions of a point Pw:  g[j] = Pw[j] / voxel - 0.5 (float64; the quotient is the one cell[j] is the floor of),
 *     B[j] = floor(g[j]),  fr[j] = (float) (g[j] - B[j]).  The nearest voxel cell is one of the eight corners.
 *     Corner c is KNOWN when its three indices lie in [-2^20, 2^20) (no wrap: a corner at -2^20 - 1 or 2^20 is missing), its key
 *     is found by the read-only probe and its record has n >= min_frames and n > 0; then v_c = S / (float) n.
 *   tri(v) of eight values and fr, in this order (x, then y, then z):
 *     x00 = lerp(v0, v1, fr[0]), x10 = lerp(v2, v3, fr[0]), x01 = lerp(v4, v5, fr[0]), x11 = lerp(v6, v7, fr[0]);
 *     y0 = lerp(x00, x10, fr[1]), y1 = lerp(x01, x11, fr[1]);  tri = lerp(y0, y1, fr[2]).
 *   Sampling.  interp = 0, and every coarse-mode sample: D is the nearest voxel's, as m4d_tsdf_raycast's.  interp = 1, a KNOWN
 *     sample in fine mode: D = tri(v) at the sample's Pw when all eight corners are KNOWN, else the nearest voxel's value.  The hit
 *     test and z* = z_{i-1} + hv * (double) (prev / (prev - D)) are unchanged.  With interp = 0 depth_out and hits are
 *     m4d_tsdf_raycast's bit for bit.
 *   At a hit (either interp; computed when an output needs it): P* = the ray's point at the float64 z* (X = ax * z*, Y = ay * z*,
 *     Pw as above), with its base cell, fractions and corners.
 *     normal: only when all eight corners are KNOWN.  The gradient of the interpolant, float32:
 *       gx = lerp(lerp(v1 - v0, v3 - v2, fr[1]), lerp(v5 - v4, v7 - v6, fr[1]), fr[2])
 *       gy = lerp(lerp(v2 - v0, v3 - v1, fr[0]), lerp(v6 - v4, v7 - v5, fr[0]), fr[2])
 *       gz = lerp(lerp(v4 - v0, v5 - v1, fr[0]), lerp(v6 - v2, v7 - v3, fr[0]), fr[1])
 *     widened; into the camera frame c[j] = (R[0][j] gx + R[1][j] gy) + R[2][j] gz; len = sqrt((c0 c0 + c1 c1) + c2 c2);
 *     n[j] = (float) (c[j] / len).  The field grows towards free space, so n faces the camera on a front face.  len not > 0 (zero
 *     or NaN) or a corner that is not KNOWN: the three floats are the quiet NaN 0x7FC00000.
 *     colour: m_c[k] = ((float) s_k / (float) nc) / 255.0f of a record, s = sr, sg, sb.  All eight corners KNOWN with nc > 0:
 *     tri(m[k]) per channel.  Otherwise the nearest voxel of P* (cell = floor(Pw / voxel), in range) when KNOWN with nc > 0: its
 *     m[k].  Otherwise three quiet NaNs.
 *     view: vl = sqrt((ax ax + ay ay) + 1.0), dot = ((n0 ax + n1 ay) + n2) / vl on the widened float32 normal,
 *     shade = (float) (0.25 + 0.75 * fmax(0.0, -dot)), 1.0f where the normal is missing; byte k = m4d_depth_export's rgb rule of
 *     (colour[k] * shade), a missing colour counting as 0.5f.
 *   A miss (a sample with a non-finite pose included): depth_out as m4d_tsdf_raycast's (fill applies to depth_out only), normal_out
 *     and colour_out three quiet NaNs, view_out 0, 0, 0.
 * A thread probes the eight corners of a base cell together (the eight first-slot key loads, then the eight (S, n) loads; the
 * sequential probe only for a corner whose first slot holds another key) and keeps them while B does not change; the 16 colour
 * bytes of a record are read only at a hit.  Neither changes a bit.
 * Returns 1 without a launch for what m4d_tsdf_raycast refuses, interp outside 0..1, a normal / colour / view stride smaller than
 * 3 h w, normal_out / colour_out off 4 bytes.  Plain launch (capturable).  Additive entry point: ABI 6 unchanged. */
int m4d_tsdf_render(const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c, const double* pose,
                    int h, int w, float near, float far, float voxel, int trunc, int min_frames,
                    const float* guide, long long guide_stride, int window,
                    const float* fill, long long fill_stride, int interp,
                    float* depth_out, long long out_stride, float* normal_out, long long normal_stride,
                    float* colour_out, long long colour_stride, uint8_t* view_out, long long view_stride,
                    void* hits, void* stream);

/* ---- training summaries (main.py --mode=train --log_dir): float32 maps -> the uint8 images of a TensorBoard event -------- */

/* Up to 16 float32 maps of different sizes -> uint8 images, in one launch.  src, stride, h, w, c, kind and out_offset are
 * HOST arrays of n_maps entries (the descriptors travel to the kernel by value: no device-side table).  Map m is
 * [b_m, h[m], w[m], c[m]] with c 1 or 3, image i at src[m] + i * stride[m] ELEMENTS (stride >= h*w*c: a frame slice of a
 * [b,T,H,W,c] batch is read in place); only the first n images of every map are converted (tf.summary.image's max_outputs;
 * every map must hold at least n).  The byte of map m, image i < n, pixel (y,x), channel ch is
 *   out[out_offset[m] + ((i*h + y)*w + x)*c + ch]
 * float32, one IEEE rounding per operation:
 *   q(v)    : v NaN -> 0; t = v * 255.5f; t < 0 -> 0; t >= 255 -> 255 (+inf included); else (uint8) t, truncated.  This is
 *             TensorFlow's convert_image_dtype(float32 -> uint8, saturate=True) -- scale by max + 0.5, saturate, truncating
 *             cast -- which tf.summary.image applies.  Stated from TensorFlow's source as remembered: nothing in the build
 *             environment can execute TensorFlow, so the rule is NOT checked against it.
 *   kind 0  : colour or any map already in [0,1]: q(v)
 *   kind 1  : log depth (m4depth_network.py:403,409,411-414):
 *             q(logf(fminf(fmaxf(d, 1.0f), 200.0f)) / 5.29831737f), the constant the float32 nearest to ln 200; NaN, 0,
 *             negative depths and velodyne holes give 0.
 * Every output byte of the n images is written, nothing else.  Returns 1 without a launch for: n_maps outside 1..16, n < 1,
 * a NULL array, source or out, c not 1 or 3, an unknown kind, h or w < 1, a stride smaller than an image, a float pointer off
 * 4 bytes, a negative out_offset or overlapping output ranges.  Plain launch (capturable).  Additive entry point: ABI 6
 * unchanged. */
int m4d_summary_images(int n_maps, const float* const* src, const long long* stride, const int* h, const int* w, const int* c,
                       const int* kind, const long long* out_offset, int n, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* M4DEPTH_HIP_H_ */
