/*
 * m4depth_hip_experiments.h -- entry points that exist ONLY in a `make -C m4depth_amd/csrc EXPERIMENTS=1` build of
 * libm4depth_hip.so (m4d_build_info() then says "+experiments").  The alternative kernels here were measured, found not to
 * be faster end to end, and are NOT dispatched by the product (DESIGN_HISTORY.md); they stay buildable for the bit-identity
 * tests and the profiling tools that compare against them.  The profiling hooks at the end make kernels write cycle stamps or
 * counters into a buffer the CALLER sizes; the product's kernels do not contain them.  Selectors and hooks are PROCESS-WIDE
 * state: set them from one thread, while nothing is launching.
 */
#ifndef M4DEPTH_HIP_EXPERIMENTS_H_
#define M4DEPTH_HIP_EXPERIMENTS_H_

#ifdef __cplusplus
extern "C" {
#endif

/* Which kernel serves m4d_conv3x3_wino6_bias_act (results are bit-identical): 0 (default) and 1 = the 16x16-pixel x 64-cout
 * workgroups of m4d_wino6.hip, 2 = the wide kernel of m4d_wino6w.hip (16x16 pixels x all 96 / 128 couts, two passes over the
 * Winograd position rows) wherever it applies (64 < Cout <= 128, Cout % 4 == 0), 3 = the half-tile kernel of m4d_wino6h.hip
 * (16x8 pixels x 64 couts per workgroup) everywhere. */
void m4d_wino6_set_variant(int variant);
/* Under variant 0 the half-tile kernel serves the launches whose m4d_wino6.hip grid would have at most `max_wg` workgroups
 * (default 0 = none: faster alone on small grids, no gain inside the frame pipeline). */
void m4d_wino6_set_half_tile_max_workgroups(int max_wg);

/* m4d_voxel_map_integrate (include/m4depth_hip.h) without the in-wave combining of equal keys: every vertex probes the table and
 * issues its own atomics.  Same arguments, same bits; what tools/bench_voxel_map.py measures the product kernel against. */
int m4d_voxel_map_integrate_uncombined(const void* vertices, const int* counts, int b, int cap, float voxel, long long stamp,
                                       void* state, int log2_slots, void* stream);

/* m4d_tsdf_allocate (include/m4depth_hip.h) without the per-thread skip of a key that equals the previous one: every sample of
 * every ray probes the table.  Same arguments, same key set; what tools/bench_tsdf_mesh.py measures the product kernel against. */
int m4d_tsdf_allocate_plain(const float* depth, long long depth_stride, const float* cam_f, const float* cam_c, const double* pose,
                            int b, int h, int w, float near, float far, float voxel, int trunc, void* state, int log2_slots,
                            void* stream);

/* m4d_tsdf_raycast (include/m4depth_hip.h) in the forms its two choices were measured against: variant bit 0 = a wave is an 8x8
 * pixel tile (clear: 64 consecutive pixels of the raster), bit 1 = no probe for a key the previous sample of the ray had (clear:
 * every sample probes).  0 is the plain kernel, 3 the product's; anything else is refused.  The other arguments and every bit of
 * the result are m4d_tsdf_raycast's; what tools/bench_tsdf_raycast.py measures the product kernel against. */
int m4d_tsdf_raycast_plain(int variant, const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c,
                           const double* pose, int h, int w, float near, float far, float voxel, int trunc, int min_frames,
                           const float* guide, long long guide_stride, int window, const float* fill, long long fill_stride,
                           float* depth_out, long long out_stride, void* hits, void* stream);

/* m4d_tsdf_render (include/m4depth_hip.h) in the forms its two devices were measured against: variant bit 0 = the eight corners
 * of a base cell are probed together (clear: eight read-only probes back to back), bit 1 = the corners are kept while the base
 * cell does not change (clear: every fine sample probes).  0 is the plain kernel, 3 the product's; anything else is refused.
 * The other arguments and every bit of the result are m4d_tsdf_render's (tools/bench_tsdf_raycast.py). */
int m4d_tsdf_render_plain(int variant, const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c,
                          const double* pose, int h, int w, float near, float far, float voxel, int trunc, int min_frames,
                          const float* guide, long long guide_stride, int window, const float* fill, long long fill_stride,
                          int interp, float* depth_out, long long out_stride, float* normal_out, long long normal_stride,
                          float* colour_out, long long colour_stride, uint8_t* view_out, long long view_stride,
                          void* hits, void* stream);

/* ---- launch tape (csrc/m4d_tape.hip): a recorded sequence of this library's kernel launches, replayed as PLAIN STREAM
 * LAUNCHES from one host loop -- the host-side cost of a hipGraph replay without its effect on concurrent small kernels
 * (DESIGN_HISTORY.md).  Between m4d_tape_begin()
 * and m4d_tape_end() every entry point called BY THE SAME THREAD records its launches (function, grid, block, LDS, a copy of
 * every argument) instead of executing them; the recording pass must run on the buffers the replays will use.
 * m4d_tape_begin returns the tape id (-1: already recording), m4d_tape_end the number of launches recorded,
 * m4d_tape_replay issues them on `stream` in order (0 or a hipError_t). */
int m4d_tape_begin(void);
int m4d_tape_end(void);
int m4d_tape_length(int tape);
int m4d_tape_replay(int tape, void* stream);
int m4d_tape_free(int tape);
/* The scatter backwards (m4d_backproject_bwd, m4d_dscv_bwd) zero their outputs with a kernel launch (m4d_zero_f32), which
 * is recorded like any other launch. */

/* ---- profiling hooks: NULL (the default) switches a hook off; results are unchanged while one is on.  The buffer must hold
 * what the hook's description says for the launch that follows -- the kernels do not know its size. */
/* Winograd kernel 4 of m4d_conv3x3_wino2_bias_act (tools/wino4_phases.py): 202 uint64 per workgroup (first 512 of batch item
 * 0) = cycle counter of wave 0 at kernel entry / end of the K loop, per K chunk (first 40) at five phase boundaries, and (last
 * word) at the end of the epilogue. */
void m4d_wino_set_stamps(unsigned long long* device_buffer);
/* m4d_conv3x3_wino6_bias_act on the one-workgroup-per-unit kernel (tools/wino6_phases.py): 1280 uint64 for each of the first
 * 64 workgroups, per-position cycle stamps of every wave.  While set, every launch takes that kernel. */
void m4d_wino6_set_stamps(unsigned long long* device_buffer);
/* The fused level front (tools/bench_kernels.py): 8 uint64 per workgroup, 7 phase cycle stamps. */
void m4d_front_set_stamps(unsigned long long* device_buffer);
/* The hypothesis-per-lane DSCV kernels (m4d_dscv_set_variant 3 / 4): 6 uint64 per workgroup = cycle counter at entry / after
 * the box reduction / after window staging / at exit, window pixels, window width. */
void m4d_dscv_set_stamps(unsigned long long* device_buffer);
/* The DSCV window kernels (variants 2-4): a device uint32 incremented by every workgroup whose footprint box did not fit the
 * LDS window. */
void m4d_dscv_set_fallback_counter(unsigned int* device_counter);

#ifdef __cplusplus
}
#endif
#endif /* M4DEPTH_HIP_EXPERIMENTS_H_ */
