/* knerf_debug.h -- diagnostics for tests/ and tools/ only, built into libknerf_probe.so (keras_nerf_amd/build.py).
 *
 * Nothing here is part of the product ABI (include/knerf.h) and the product library does not contain it: layout-table
 * introspection for the CPU-side lane simulator (tests/test_layout_sim.py), views of a context's workspaces for kernel-level
 * parity tests, the hardware-fact probes of tests/test_gpu_probe.py and the bandwidth / MFMA-rate probes of tools/.
 * libknerf_probe.so links against libknerf_hip.so (same directory) and shares its internal context layout (csrc/ctx.h).
 */
#ifndef KNERF_DEBUG_H
#define KNERF_DEBUG_H
#include "knerf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kind 0: forward A-fragment table, 1: forward bias table, 2: dgrad A-fragment table, 3: wgrad destination tables
 * (concatenated), 4: offsets of the jobs inside kind 3.  Entries of 0..2 index the extended weight buffer (parameters, then the
 * composed head matrix [288][4] and its bias [4]; csrc/layout.h) or are -1; entries of 3 index the flat gradient, or
 * param_count + i for element i of the head accumulator, or are -1.  kind + 16 k: the same for entry k of the built-in trunk shapes
 * (csrc/layout.h KNERF_FUSED_SHAPES; composed head [dense_units + 32][4]); kind 5 + 16 k: {n_layers, skip_layer, dense_units,
 * param_count, pos_emb_xyz, pos_emb_dir} of entry k; an index behind the last entry fails.  Pass out=NULL to query the length.  No device needed. */
int knerf_debug_table(int kind, int32_t* out, size_t* n);
/* the general-shape path's layer program for a config (no device needed): 16 int32 per Dense layer in Keras order =
 * {kernel offset, bias offset, fan_in, fan_out, padded input width, padded output width, n_seg, seg0 (buffer col0, width,
 * kernel row0), seg1 (...), relu, head (-1 | 0 sigma | 1 rgb), padded width of the output buffer or -1}. */
int knerf_debug_generic_plan(const knerf_config* cfg, int32_t* out, size_t* n);
/* device buffers of the last knerf_train_chunk for kernel-level tests: 0 act, 1 mask, 2 dz, 3 raw, 4 draw,
 * 5 merged fine t-values, 6 coarse weights, 7 extended weight buffer of `net` (parameters + composed head); on a context of the
 * general-shape path (csrc/generic.h): 8 all activation buffers, 9 all dZ buffers of the last pass (0-2 belong to the fused path) */
int knerf_debug_buffer(knerf_ctx* ctx, int net, int which, void** dev, size_t* bytes);
/* hardware-fact probes: kind 0 = one v_mfma_f32_32x32x16_bf16 (in0 = A fragments [64][8] bf16, in1 = B fragments,
 * out = [64][16] f32); kind 1 = one ds_read_b64_tr_b16 (in0 = 4 KiB LDS image, in1 = [64] int32 byte offsets,
 * out = [64][4] u16).  All device pointers. */
int knerf_debug_probe(int kind, const void* in0, const void* in1, void* out, void* stream);
/* HBM write-pattern probe: `workgroups` x 8 waves each store `blocks` 1 KiB blocks into tiles `tile_stride` bytes apart;
 * mode 0 = the chain kernels' pattern, 1 = the 8 waves of a workgroup interleaved. */
int knerf_debug_write_probe(void* out, int workgroups, int blocks, long long tile_stride, int mode, int spin, void* stream);
/* HBM read-pattern probe: each of workgroups x 8 waves streams bytes_per_wave contiguous bytes in 1 KiB instructions;
 * mode 0 = nt LDS-DMA (wgrad's loads), 1 = plain register loads. */
int knerf_debug_read_probe(const void* in, int workgroups, long long bytes_per_wave, int mode, void* out, void* stream);
/* MFMA-shape rate probe (shape 32: v_mfma_f32_32x32x16_bf16, 16: v_mfma_f32_16x16x32_bf16) with the chain kernels' operand
 * traffic; `blocks` workgroups of 512 threads, 96 * 2^15 * 16 FLOP per wave and iteration. */
int knerf_debug_rate_probe(int shape, const void* in0, const void* in1, void* out, int blocks, int iters, void* stream);
/* The compositing kernel's training half on caller-made inputs, without a context (csrc/composite.hip; CompositeArgs of
 * csrc/kernels.h): raw [R,S,4], t [R,S], target [R,3] -> image [R,3], depth [R], weights [R,S], draw [R,S,4] and *loss +=
 * loss_scale * sum of squared differences.  loss_partial [ceil(R/4)] or null: the deterministic mode's per-workgroup terms, added in a
 * fixed order by the loss-reduction kernel behind the compositing kernel (as knerf_train_chunk does) instead of one atomic per
 * workgroup.  tile_flags [R*S/32] or null; tile_list [R*S/32] with tile_count (one int, the caller sets it to zero) or both null;
 * tile_list2 [*tile_count2 + R*S/32] with tile_count2 and tile_off2, only together with tile_list, or both null.  Tile outputs need
 * S % 32 == 0.  All pointers are device pointers; 1 <= S <= 1024. */
int knerf_debug_composite_train(void* stream, const float* raw, const float* t, const float* target, int n_rays, int n_samples,
                                int white_background, float grad_scale, float loss_scale, float* image, float* depth, float* weights,
                                float* draw, float* loss, float* loss_partial, int* tile_flags, int* tile_list, int* tile_count,
                                int* tile_list2, int* tile_count2, int tile_off2);
/* The same on the EXTENDED compositing kernel (csrc/composite_ext.hip; include/knerf.h knerf_set_objective), always -- also for
 * KNERF_LOSS_MSE without a regulariser, where the product takes the plain kernel.  obj: the record (`nets` is not read: the weights
 * apply to this pass); reg_scale: inv_chunks / R of knerf_train_chunk; terms [4] (photometric, squared error, distortion, entropy;
 * added to); terms_partial [4][ceil(R/4)], given exactly when loss_partial is: the deterministic mode's per-workgroup terms. */
int knerf_debug_composite_objective(void* stream, const float* raw, const float* t, const float* target, int n_rays, int n_samples,
                                    int white_background, float grad_scale, float loss_scale, float* image, float* depth, float* weights,
                                    float* draw, float* loss, float* loss_partial, int* tile_flags, int* tile_list, int* tile_count,
                                    int* tile_list2, int* tile_count2, int tile_off2, const knerf_objective* obj, float reg_scale,
                                    float* terms, float* terms_partial);
/* The deterministic mode's tile compaction (one workgroup): list = the ascending indices i in [0, n) with flags[i] != 0 and
 * (i % period) < real, *count = their number, stats[0] += *count, stats[1] += the number of i with (i % period) < real; stats may
 * be null.  list holds up to n entries.  All pointers are device pointers. */
int knerf_debug_compact_tiles(const int* flags, int n, int period, int real, int* list, int* count, long long* stats, void* stream);

/* ---- the general-shape path's four matmul kernels on caller-made buffers (csrc/generic.hip; tests/test_gpu_generic_gemm.py) ----
 * Which kernel and grid the launchers pick, from the host arithmetic they use themselves (no device needed).
 * what 0, a GEMM over (M = m_or_steps, N, K): out = {1 weights-stationary gemm_ws_kernel | 0 streaming gemm_kernel, NT, gx, gy,
 * LDS bytes, LDS row pitch, 0, 0}; a wave of the persistent kernel walks row tiles w, w + 8 gx, ... of M / 32.
 * what 1, a weight gradient over (steps = m_or_steps, N, K): out = {1 wgrad_coop_kernel | 0 wgrad_kernel<KT, NT>, gx, gy, gz, KT,
 * NT, partial slabs per block, floats per slab}; per_wave != 0: the per-wave kernel whatever the product would pick. */
int knerf_debug_generic_launch(int what, long long m_or_steps, int N, int K, int per_wave, int32_t out[8]);
/* floats of `partial` a deterministic weight-gradient launch over a [K] x [N] layer needs (any number of steps) */
int knerf_debug_generic_wgrad_partial_floats(int K, int N, int per_wave, size_t* floats);
/* One launch_gemm: C[M][N] = A[M][K] . Bt[N][K]^T (+ bias[col < n_real]) (relu) (* relu bit).  bf16 buffers are uint16.  Device
 * pointers with the element count of each buffer; Cb is the buffer's BASE and the output starts at column c_col0 of its rows.
 * Exactly one of Cb / Cf; mask_out (forward) or mask_in (dgrad: no bias, no relu) go with Cb.  live: a HOST array of n_live
 * 32-row tile indices in [0, M / 32), or n_live = -1 for every tile; live_dev: device scratch of at least n_live + 1 int32 that
 * receives {count, entries}.  Every argument is checked on the host against what the launch can address -- M a multiple of 128,
 * N and K of 32, leading dimensions of 8 and >= the width, 16-byte aligned bases, ldc and c_col0 multiples of NT, mask_cols >= N / 8,
 * every buffer long enough for the last row -- and KNERF_ERR_INVALID comes back before any HIP call. */
typedef struct knerf_debug_gemm {
    const uint16_t* A; size_t a_elems; int lda;
    const uint16_t* Bt; size_t bt_elems; int ldb;
    long long M; int N, K;
    const float* bias; size_t bias_elems; int n_real;
    int relu;
    unsigned char* mask_out; const unsigned char* mask_in; size_t mask_bytes; int mask_cols;
    uint16_t* Cb; size_t cb_elems; int ldc, c_col0;
    float* Cf; size_t cf_elems; int ldcf;
    const int32_t* live; long long n_live; int32_t* live_dev; size_t live_dev_elems;
} knerf_debug_gemm;
int knerf_debug_generic_gemm(void* stream, const knerf_debug_gemm* args);
/* One launch_wgrad (and its ordered reduce pass when `partial` is given): grad[w_off + row n_real + n] += sum_m X[m][k] Z[m][n]
 * for the kernel rows `row` the segments {buffer col0, width, kernel row0} x n_seg map column k to and n < n_real,
 * grad[b_off + n] += sum_m Z[m][n]; m over steps x 32 rows or over the live list (as above, entries in [0, steps); strictly ascending
 * when `partial` is given).  selector 0: the kernel the product picks, 1: the per-wave wgrad_kernel.  partial: null (fp32 atomics)
 * or at least knerf_debug_generic_wgrad_partial_floats floats.  Checked like knerf_debug_generic_gemm; segments must lie inside K
 * and every destination inside grad_elems. */
typedef struct knerf_debug_wgrad {
    const uint16_t* X; size_t x_elems; int ldx;
    const uint16_t* Z; size_t z_elems; int ldz;
    long long steps; int N, K;
    float* grad; size_t grad_elems;
    int w_off, b_off, n_real;
    int n_seg; int seg[6];
    float* partial; size_t partial_elems;
    const int32_t* live; long long n_live; int32_t* live_dev; size_t live_dev_elems;
    int selector;
} knerf_debug_wgrad;
int knerf_debug_generic_wgrad(void* stream, const knerf_debug_wgrad* args);
/* the argument check of the two entry points above on its own (what 0: a knerf_debug_gemm, 1: a knerf_debug_wgrad): KNERF_OK or
 * KNERF_ERR_INVALID; never touches the device or the pointers' targets other than the host live list */
int knerf_debug_generic_check(int what, const void* args);

#ifdef __cplusplus
}
#endif
#endif /* KNERF_DEBUG_H */
