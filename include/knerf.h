/* knerf.h -- C ABI of libknerf_hip.so: the MI355X (gfx950) NeRF train/render hot path.
 *
 * The reference (naufalso/keras_nerf) has no FFI layer: its hot path is the Python class surface
 * keras_nerf/model/nerf/{nerf,utils,mlp}.py on stock TensorFlow ops.  Each entry point below names the reference
 * code it replaces; the modules under keras_nerf_amd/model/nerf bind them with ctypes behind the reference's class names.
 *
 * Conventions: every function returns 0 on success or a negative knerf_status; knerf_last_error() gives the text.
 * All array arguments are DEVICE pointers to contiguous row-major fp32 unless marked host.  `stream` is a
 * hipStream_t (may be NULL).  Nothing is retained past a call; the context owns weights, gradients, Adam slots
 * and workspaces.  One context per GPU, not thread safe.
 */
#ifndef KNERF_H
#define KNERF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct knerf_ctx knerf_ctx;

typedef enum knerf_status {
    KNERF_OK = 0,
    KNERF_ERR_INVALID = -1,       /* bad argument / unsupported architecture                      */
    KNERF_ERR_HIP = -2,           /* a HIP runtime call failed                                    */
    KNERF_ERR_NONFINITE = -3,     /* a gradient is not finite (reference: assert_all_finite)      */
    KNERF_ERR_NODEVICE = -4       /* no gfx950 device visible                                     */
} knerf_status;

/* NeRF(...) constructor arguments (reference nerf.py:11-14) + compile() arguments (nerf.py:78) + Adam defaults
 * of tf.keras.optimizers.get('adam') (nerf.py:163-165). */
typedef struct knerf_config {
    int32_t n_coarse, n_fine;          /* 64, 128; 2 <= n_coarse <= 512, n_coarse + n_fine <= 1024 */
    int32_t pos_emb_xyz, pos_emb_dir;  /* 10, 4   */
    int32_t n_layers, dense_units, skip_layer; /* 8, 256, 4; fused kernels: the triples of csrc/layout.h KNERF_FUSED_SHAPES (widths 256, 128; 64 at build time); others: csrc/generic.hip */
    int32_t white_background;          /* compile(white_background=...) */
    int32_t oob_clamp;                 /* 0: out-of-range mid-point gather yields 0 (tf.gather on GPU); 1: clamp */
    float lr, beta1, beta2, epsilon;   /* 1e-3, 0.9, 0.999, 1e-7 */
    int32_t flags;                     /* KNERF_FLAG_* */
} knerf_config;

/* KNERF_FLAG_FORCE_GENERIC: run a shape the fused kernels cover through the general-shape kernels too (tests compare the two paths).
 * KNERF_FLAG_ENCODED_WIDTHS: a stand-alone NeRFMLP (reference mlp.py:4-59; tests/model/nerf/test_nerf_mlp.py:6-45 feeds 99-wide
 *   tensors to BOTH inputs).  Keras Dense takes its input size from the last dimension of the first call (mlp.py:11-27 names
 *   none), so the two widths are free: with this flag pos_emb_xyz / pos_emb_dir hold the encoded input WIDTHS themselves
 *   (1..4096 each, not the number of frequencies) and n_coarse / n_fine are ignored.  Such a context serves knerf_set_weights /
 *   knerf_get_weights / knerf_weights_device / knerf_mlp_call only; the ray entry points return KNERF_ERR_INVALID. */
enum { KNERF_FLAG_FORCE_GENERIC = 1, KNERF_FLAG_ENCODED_WIDTHS = 2 };

enum { KNERF_COARSE = 0, KNERF_FINE = 1 };

/* number of trainable scalars per MLP (595,844 for the default shape; reference mlp.py:11-27) */
size_t knerf_param_count(void);
/* the same for any NeRFMLP(n_layers, dense_units, skip_layer) with pos_emb_xyz / pos_emb_dir (mlp.py:11-27); 0 = invalid.
 * Shapes outside csrc/layout.h KNERF_FUSED_SHAPES run on the general-shape kernels (csrc/generic.hip): same API, same numerics contract. */
size_t knerf_param_count_for(const knerf_config* cfg);

int knerf_create(const knerf_config* cfg, knerf_ctx** out);
int knerf_destroy(knerf_ctx* ctx);
const char* knerf_last_error(const knerf_ctx* ctx);   /* ctx may be NULL: error of the last failed create */

/* Weights of one MLP as ONE flat fp32 vector in Keras trainable_variables order
 * (layer_0/kernel[in,out], layer_0/bias, ..., sigma, features, rgb_features, rgb); HOST pointers.
 * Replaces NeRFMLP weight creation / load_weights / save_weights (nerf.py:116-136, 45-64). */
int knerf_set_weights(knerf_ctx* ctx, int net, const float* host_flat, size_t n);
int knerf_get_weights(knerf_ctx* ctx, int net, float* host_flat, size_t n);
/* device views for collectives: weights of one net; the gradient accumulators of BOTH nets as one buffer
 * [coarse | fine] (2*param_count floats) so that a single all-reduce covers the step (train.py:75). */
int knerf_weights_device(knerf_ctx* ctx, int net, float** dev, size_t* n);
int knerf_grads_device(knerf_ctx* ctx, float** dev, size_t* n);
/* re-derive the bf16 MFMA weight streams from the fp32 master weights (after an external write to them) */
int knerf_refresh_weights(knerf_ctx* ctx, void* stream);

/* NeRF._predict_and_render_chunk (nerf.py:175-216) for one net on given t-values:
 * encode -> MLP -> composite.  o,d [R,3]; t [R,S]; outputs image [R,3], depth [R], weights [R,S]. */
int knerf_forward_chunk(knerf_ctx* ctx, void* stream, int net, const float* o, const float* d, const float* t,
                        int n_rays, int n_samples, float* image, float* depth, float* weights);

/* NeRFMLP.__call__((xyz_enc, dir_enc)) (mlp.py:29-50) on inputs that are ALREADY positional encodings:
 * xyz_enc [n, 3+6*pos_emb_xyz], dir_enc [n, 3+6*pos_emb_dir] (or [n, pos_emb_xyz], [n, pos_emb_dir] on a context created with
 * KNERF_FLAG_ENCODED_WIDTHS) fp32 device pointers; raw [n,4] = (rgb after sigmoid, sigma after relu).  The reference calls its MLPs this way only to create weights and in a shape test; it runs on the
 * general-shape kernels (bf16 operands, fp32 accumulate) for every shape, including the default one. */
int knerf_mlp_call(knerf_ctx* ctx, void* stream, int net, const float* xyz_enc, const float* dir_enc, uint64_t n, float* raw);

/* the fine branch's sampling (nerf.py:182-191, utils.py:60-97): t_out [R, n_coarse+n_fine] sorted.
 * u [R,n_fine] in [0,1) or NULL for the built-in Philox stream keyed by (seed, stream_id, ray_offset + ray). */
int knerf_sample_fine(knerf_ctx* ctx, void* stream, const float* t_coarse, const float* w_coarse, const float* u,
                      uint64_t seed, uint64_t stream_id, uint64_t ray_offset, int n_rays, float* t_out);

/* NeRF.predict_and_render_chunk (nerf.py:218-227): coarse pass, sampling, fine pass. Any output may be NULL
 * except the two images.  t_fine [R, n_coarse+n_fine] receives the merged t-values. */
int knerf_render_chunk(knerf_ctx* ctx, void* stream, const float* o, const float* d, const float* t, const float* u,
                       uint64_t seed, uint64_t ray_offset, int n_rays,
                       float* c_image, float* c_depth, float* c_weights,
                       float* f_image, float* f_depth, float* f_weights, float* t_fine);

/* predict_and_render_images (nerf.py:229-304): the chunk loop of knerf_render_chunk over n_rays = C * ray_chunks rays in one
 * host call; outputs are whole-batch arrays ([n_rays, ...], images mandatory, the rest optional; t_fine [n_rays,
 * n_coarse+n_fine] receives the merged t-values of nerf.py:190-191).  ray_offset of chunk i is i * ray_chunks, so results
 * equal C separate knerf_render_chunk calls. */
int knerf_render_batch(knerf_ctx* ctx, void* stream, const float* o, const float* d, const float* t, const float* u, uint64_t seed,
                       int n_rays, int ray_chunks, float* c_image, float* c_depth, float* c_weights, float* f_image, float* f_depth,
                       float* f_weights, float* t_fine);

/* One iteration of train_step's chunk loop (nerf.py:351-421): coarse forward+backward, fine forward+backward,
 * gradients accumulated as acc += g * inv_chunks, chunk losses accumulated into loss[0] (coarse) / loss[1] (fine)
 * (device, 2 floats, caller zeroes them per step).  target [R,3]. */
int knerf_train_chunk(knerf_ctx* ctx, void* stream, const float* o, const float* d, const float* t,
                      const float* target, const float* u, uint64_t seed, uint64_t ray_offset, int n_rays,
                      float inv_chunks, float* loss, float* c_image, float* f_image);

/* The whole chunk loop of train_step (nerf.py:351-421) in one call: n_rays must be a multiple of ray_chunks (the
 * reference's assert, nerf.py:100); chunk i covers rays [i*ray_chunks, (i+1)*ray_chunks) with weight 1/C.  Same arguments
 * as knerf_train_chunk, arrays sized for all n_rays. */
int knerf_train_batch(knerf_ctx* ctx, void* stream, const float* o, const float* d, const float* t, const float* target,
                      const float* u, uint64_t seed, int n_rays, int ray_chunks, float* loss, float* c_image, float* f_image);

/* coarse_optimizer.apply_gradients + fine_optimizer.apply_gradients + accumulator reset (nerf.py:455-471).
 * Call after the optional all-reduce of knerf_grads_device().  ASYNCHRONOUS: the finite check of nerf.py:381-382 runs on the
 * device in front of the update, and a step whose gradient is not finite leaves weights and Adam slots untouched (the
 * accumulators are zeroed either way).  The host learns of it from knerf_poll_nonfinite. */
int knerf_apply_adam(knerf_ctx* ctx, void* stream);
/* Returns KNERF_ERR_NONFINITE once for every batch of skipped steps since the previous poll (and takes them back out of the
 * step counter), KNERF_OK otherwise.  wait != 0 synchronises `stream` first, i.e. covers every knerf_apply_adam issued so far;
 * wait == 0 reads the device-written status word as it stands (steps that have completed). */
int knerf_poll_nonfinite(knerf_ctx* ctx, void* stream, int wait);
int knerf_zero_grads(knerf_ctx* ctx, void* stream);

/* Run-time options of a context (no environment variables are read by the library).  Names:
 *   "deterministic"     0/1  weight gradients and losses without floating-point atomics: every workgroup writes its partial sums
 *                            to its own slab and an ordered second pass adds them, so two runs of the same step are bit-identical
 *                            (slower; the reference's TF ops give no such guarantee either -- this is a test/diagnosis mode).  Both MLP paths: the
 *                            fused kernels and, since round 5, the general-shape kernels (csrc/generic.hip).
 *   "skip_dead_tiles"   0/1  (default 1) the backward kernels skip every 32-sample tile whose dL/d(rgb, sigma) is EXACTLY zero for all samples
 *                            (empty space with a closed ReLU gate on sigma, rays whose pixel error is exactly 0): such samples add
 *                            exactly nothing to any of the 48 gradient tensors (utils.py:36-45, mlp.py:40), so the result is the
 *                            same; applies when n_coarse and n_coarse + n_fine are multiples of 32 (every MLP shape: the fused kernels
 *                            and, since round 5, the general-shape kernels walk the list of live tiles).
 *   "grad_diagnostics"  0/1  (default 0) knerf_train_batch counts the non-zero entries of the last chunk's gradient of each net
 *                            (knerf_grad_diagnostics; the reference does this when run_eagerly, nerf.py:430-451); one launch of the
 *                            coarse weight-gradient kernel per chunk while it is on.
 *   "merge_render_rays" 0..1048576 (default 65536) the same for knerf_render_batch on the fused kernels (rendering keeps no saved
 *                            tensors: 5 KB of workspace per ray; outputs bit-identical for every value); the general-shape kernels
 *                            render under "merge_chunk_rays".
 *   "merge_chunk_rays"  0..1048576 (default 4096) knerf_train_batch runs m consecutive chunks as one set of launches,
 *                            m the largest divisor of the chunk count with m * ray_chunks <= this value (0: every chunk its own
 *                            launches).  `ray_chunks` is the reference's memory knob (nerf.py:100, 332-473): every ray's forward, loss
 *                            term and gradient contribution is independent of the chunk that holds it (mean over R rays times 1 / C
 *                            = mean over m R rays times m / C; the fine sampler's random numbers are keyed by the ray's index in the
 *                            batch), so rendered outputs are bit-identical and accumulated gradients equal up to the order of fp32
 *                            sums.  4,096 rays need 8 GB of workspace here; if that cannot be allocated the caller's own chunk
 *                            size is used -- by knerf_render_batch too -- and remembered for that (ray_chunks, chunk count), so later
 *                            calls do not fail the same allocation again ("merge_fallbacks", read-only: how often that happened).
 *                            Off while "grad_diagnostics" is on (it counts the LAST chunk's gradient).
 *   "workspace_limit_gb" >= 0 (default 0 = off; tests) a workspace request above it is answered like an exhausted device -- by a real
 *                            failing hipMalloc -- so that the two fall-backs above can be exercised without filling the memory.
 *   "wgrad_group_max"   1..64, "wgrad_group_gb" >= 0: chunks per coarse weight-gradient launch of knerf_train_batch and the memory
 *                            budget of the workspaces that takes (defaults 4 and 40 GB; 1 or 0 = one launch per chunk).
 *   "occupancy_train"   0/1  (default 0) train passes of a net that has an occupancy grid attached skip its empty cells exactly as
 *                            render passes do (see "Empty-space skipping" below); 0, or no grid: training is unchanged, bit for bit.
 *   "termination_threshold" eps in [0, 1), finite (default 0 = off): early ray termination of the render passes (see "Early ray
 *                            termination" below); 0: renders allocate, launch and write exactly what they do without the option.
 *   "termination_segment" 1..1024 (default 32) the segment length L of early ray termination.
 *   "wgrad_cost0".."wgrad_cost<n_layers>": relative cost per sample tile of the n_layers + 1 weight-gradient jobs (nine for the default shape) (workgroups are dealt out in that
 *                            proportion; tuning sweeps).
 * knerf_get_option also answers "skip_dead_tiles_active", "wgrad_group" (of the current workspaces), "general_shape_path" and
 * "merge_fallbacks". */
int knerf_set_option(knerf_ctx* ctx, const char* name, double value);
int knerf_get_option(knerf_ctx* ctx, const char* name, double* value);
/* running totals since the last reset: 32-sample tiles the dgrad launches found live / all tiles they covered (skip_dead_tiles
 * on; both 0 otherwise).  Synchronises `stream`. */
int knerf_tile_stats(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset);
/* the same per net: live[2], total[2] = {coarse passes, fine passes} */
int knerf_tile_stats_net(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset);
/* The reference's eager-mode check "is the gradient zero" (nerf.py:430-451: tf.math.count_nonzero summed over the 24 gradient
 * tensors of each net, taken from the LAST chunk of the step).  With option "grad_diagnostics" on, knerf_train_batch keeps the sum of
 * the earlier chunks aside while the last chunk runs, counts on the device and publishes to pinned memory; this call reads
 * out[0] = coarse count, out[1] = fine count, out[2] = number of steps published so far (wait != 0: synchronises `stream` first,
 * i.e. the counts of the step just enqueued; wait == 0: of the newest step that has completed).  out: 3 values. */
int knerf_grad_diagnostics(knerf_ctx* ctx, void* stream, int wait, int64_t* out);
int knerf_step_count(const knerf_ctx* ctx);
/* Sets the count of applied steps (host mirror and device counter) and re-derives the device-side rate of the next step from it --
 * under a learning-rate schedule (knerf_set_optimizer) from the schedule. */
int knerf_set_step_count(knerf_ctx* ctx, int step);

/* ---- Optimizer options: tf.keras.optimizers.Adam(learning_rate=<schedule>, clipvalue / clipnorm / global_clipnorm, weight_decay) as
 * the reference gets it from tf.keras.optimizers.get (nerf.py:163-165).  Everything is opt-in: a context that never calls
 * knerf_set_optimizer, or calls it with a constant schedule, no clipping and no decay, runs knerf_apply_adam exactly as before (the
 * same launches, the same bits).  beta1, beta2 and epsilon stay in knerf_config.
 *   Schedule: lr(step), step = the number of steps APPLIED before this one (the first step uses lr(0), as Keras evaluates the schedule
 *     at `iterations` before incrementing; a step skipped for a non-finite gradient advances nothing), evaluated on the device in double;
 *     lr_t = lr(step) sqrt(1 - beta2^t) / (1 - beta1^t), t = step + 1.
 *       KNERF_SCHEDULE_CONSTANT     lr                                  (held as fp32, as knerf_config.lr is)
 *       KNERF_SCHEDULE_EXPONENTIAL  lr * decay_rate^(step / decay_steps); staircase != 0: the exponent is floored
 *       KNERF_SCHEDULE_COSINE       s = min(step, decay_steps); lr * ((1 - alpha) * 0.5 * (1 + cos(pi s / decay_steps)) + alpha)
 *       KNERF_SCHEDULE_PIECEWISE    values[i] for the first i with step <= boundaries[i], else values[n_values - 1]
 *                                   (n_values <= KNERF_SCHEDULE_MAX_VALUES values, n_values - 1 ascending boundaries)
 *   Clipping (clip = one KNERF_CLIP_* kind, or 0): applied to the gradient knerf_apply_adam finds in the accumulator -- after a
 *     data-parallel all-reduce, so every rank derives the same factor -- behind the finite check (whose skip rule is unchanged) and in
 *     front of the moment updates.
 *       KNERF_CLIP_VALUE        g = min(max(g, -c), c)
 *       KNERF_CLIP_NORM         per tensor (the 2 n_layers + 8 tensors of a net in Keras order): g * (c / max(|g_tensor|, c))
 *       KNERF_CLIP_GLOBAL_NORM  g * min(1, c / |g_net|) over all tensors of ONE net (the reference has one optimizer per net, so the
 *                               coarse and the fine norm are separate)
 *     Sums of squares are taken in double (any finite fp32 gradient is safe) without floating-point atomics: per-workgroup partial sums,
 *     then an ordered pass, so two runs give the same bits.  The factor is computed in double and rounded once to fp32; it is exactly
 *     1.0f where nothing is clipped.  TensorFlow multiplies by c * min(1 / |g|, 1 / c) instead: the two differ by at most one ulp of the
 *     factor.  One launch more than the plain step (the finite check is folded into the norm pass), no host synchronisation.
 *   Decoupled weight decay (Keras `weight_decay`, the AdamW form): in front of the Adam update of the same step, every parameter
 *     w -= w * fp32(weight_decay * lr(step)) -- the scheduled rate, not lr_t; the product in double on the device.  A skipped step
 *     decays nothing.
 * Element order of one step: read g, zero the accumulator, return if the step is non-finite, clip, decay, m, v, w. */
enum { KNERF_SCHEDULE_CONSTANT = 0, KNERF_SCHEDULE_EXPONENTIAL = 1, KNERF_SCHEDULE_COSINE = 2, KNERF_SCHEDULE_PIECEWISE = 3 };
enum { KNERF_CLIP_NONE = 0, KNERF_CLIP_VALUE = 1, KNERF_CLIP_NORM = 2, KNERF_CLIP_GLOBAL_NORM = 4 };   /* bits: more than one set is refused */
#define KNERF_SCHEDULE_MAX_VALUES 16
typedef struct knerf_optimizer {
    int32_t schedule;            /* KNERF_SCHEDULE_* */
    int32_t staircase;           /* exponential: 0 / 1 */
    int32_t n_values;            /* piecewise: 1..KNERF_SCHEDULE_MAX_VALUES */
    int32_t clip;                /* KNERF_CLIP_* */
    double lr;                   /* the constant rate; the initial rate of the exponential and the cosine schedule */
    double decay_steps;          /* exponential, cosine: > 0 */
    double decay_rate;           /* exponential: >= 0 */
    double alpha;                /* cosine: >= 0 */
    double clip_arg;             /* c > 0 when clip != 0 */
    double weight_decay;         /* >= 0; 0: off */
    int64_t boundaries[KNERF_SCHEDULE_MAX_VALUES - 1];   /* piecewise: ascending, >= 0 */
    double values[KNERF_SCHEDULE_MAX_VALUES];            /* piecewise: >= 0 */
} knerf_optimizer;
/* Callable at any time between steps; stream-ordered (steps enqueued earlier on `stream` keep the old settings), and the rate of
 * the next step is re-derived on the device from the DEVICE step counter, so nothing waits.  A constant schedule with no clipping and
 * no decay selects the plain kernels with knerf_config.lr replaced: a set_learning_rate for host callbacks.  KNERF_ERR_INVALID (with
 * a message) on: an unknown schedule or clip kind, two clip kinds at once, decay_steps <= 0, boundaries that do not ascend, negative
 * or non-finite numbers, n_values outside 1..KNERF_SCHEDULE_MAX_VALUES, a KNERF_FLAG_ENCODED_WIDTHS context. */
int knerf_set_optimizer(knerf_ctx* ctx, void* stream, const knerf_optimizer* opt);
int knerf_get_optimizer(knerf_ctx* ctx, knerf_optimizer* opt);
/* Adam's two slots of one net, HOST pointers to n = param_count floats each, in the layout of knerf_get_weights.  Together with
 * knerf_step_count / knerf_set_step_count and the weights this is the whole optimizer state: a context given all of it continues a
 * run bit for bit.  Both synchronise `stream`. */
int knerf_get_adam_state(knerf_ctx* ctx, void* stream, int net, float* m_host, float* v_host, size_t n);
int knerf_set_adam_state(knerf_ctx* ctx, void* stream, int net, const float* m_host, const float* v_host, size_t n);

/* ---- The objective of the train step: what tf.keras takes as `loss` in NeRF.compile beyond mean squared error, and two
 * regularisers of a ray's weights.  Opt-in: a context that never calls knerf_set_objective, or calls it with KNERF_LOSS_MSE and both
 * weights 0, runs the compositing kernel exactly as before (the same launches, the same bits).  Per ray, d_k = clip(pre_k, 0, 1) -
 * target_k, w_i the weights, acc = sum w_i, delta_i = t_{i+1} - t_i (last: 1e-10), m_i = t_i + delta_i / 2:
 *   photometric term: the mean over rays and channels of rho(d)
 *       KNERF_LOSS_MSE d^2 | KNERF_LOSS_MAE |d| (sign(0) = 0) | KNERF_LOSS_HUBER d^2 / 2 where |d| <= huber_delta, else
 *       huber_delta (|d| - huber_delta / 2) | KNERF_LOSS_LOG_COSH |d| + log1p(exp(-2 |d|)) - ln 2          (the Keras classes)
 *     its gradient passes the clip gate of the colour (pre in [0, 1], inclusive) as the squared error's does
 *   distortion (mip-NeRF 360): D = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i, evaluated in O(n) with prefix sums,
 *     which equals the definition for non-decreasing t (the contract; for unsorted t the prefix form's value is returned)
 *   opacity entropy: a = clamp(acc, 1e-4, 1 - 1e-4), H = -a ln a - (1 - a) ln(1 - a); gradient ln((1 - a) / a) inside the clamp, else 0
 * Loss of a net = photometric + distortion * mean D + opacity_entropy * mean H (means over rays); the regularisers' gradient enters
 * dL/dw directly (the weights are not clipped) and applies to the nets of `nets`.  t carries no gradient. */
enum { KNERF_LOSS_MSE = 0, KNERF_LOSS_MAE = 1, KNERF_LOSS_HUBER = 2, KNERF_LOSS_LOG_COSH = 3 };
typedef struct knerf_objective {
    int32_t loss_kind;           /* KNERF_LOSS_* */
    float huber_delta;           /* KNERF_LOSS_HUBER: > 0 */
    float distortion;            /* weight of the distortion term, >= 0; 0: off */
    float opacity_entropy;       /* weight of the opacity-entropy term, >= 0; 0: off */
    int32_t nets;                /* the regularisers apply to: 1 the coarse net, 2 the fine net, 3 both */
} knerf_objective;
/* Callable at any time between steps; stream-ordered.  Stored canonically (huber_delta 0 unless the kind is huber; nets 3 when both
 * weights are 0).  KNERF_ERR_INVALID (with a message) on: a null record, an unknown kind, huber_delta <= 0 or non-finite under
 * KNERF_LOSS_HUBER, a negative or non-finite weight, nets outside 1..3, a KNERF_FLAG_ENCODED_WIDTHS context. */
int knerf_set_objective(knerf_ctx* ctx, void* stream, const knerf_objective* obj);
int knerf_get_objective(knerf_ctx* ctx, knerf_objective* obj);
/* out: DEVICE [2][4] floats, [coarse | fine] x [photometric, mean squared error, mean D, mean H] accumulated by the passes since the
 * start of the last knerf_train_batch (which zeroes them; knerf_train_chunk adds its inv_chunks share).  All zero while the
 * objective is the plain one: the plain kernel does not compute them.  Stream-ordered copy, nothing waits. */
int knerf_objective_terms(knerf_ctx* ctx, void* stream, float* out);

/* RaysGenerator.__call__ (keras_nerf/data/rays.py:69-130) on device: c2w [B,4,4], noise [B,H,W,N] in [0,1) or
 * NULL for Philox; writes o,d [B,H,W,3] and t [B,H,W,N].  ctx may be NULL (stand-alone op). */
int knerf_generate_rays(knerf_ctx* ctx, void* stream, const float* c2w, const float* noise, uint64_t seed,
                        uint64_t stream_id, int batch, int height, int width, int n_samples, float focal,
                        float near_plane, float far_plane, float* o, float* d, float* t);

/* One training batch of rays drawn at random over ALL pixels of ALL views, in one launch: with P = n_views x height x width, slot i
 * holds pixel perm(seed, epoch)(first + i), where perm is a keyed bijection of [0, P) evaluated per slot with no table (a six-round
 * Feistel network over bit_length(P - 1) bits, round keys from Philox-4x32-10 under (seed, epoch), cycle-walked below P): the
 * positions [0, P) of one epoch visit every pixel exactly once, another epoch is another permutation, and any caller can draw any
 * slice.  Writes the pixel's ray o, d [n_rays,3] bit-identical to knerf_generate_rays for that pixel of that view, sample positions
 * t [n_rays,n_samples] jittered like knerf_generate_rays (noise [n_rays,n_samples] in [0,1), or NULL: Philox with counter
 * (n >> 2, slot, noise_stream, 2) under `seed`), target [n_rays,3] = images[v, y, x, 0:3] and, unless NULL, index [n_rays] = the
 * flat pixel index v x H x W + y x W + x.  images [V,H,W,C] with C = 3 or 4, c2w [V,4,4].  KNERF_ERR_INVALID unless
 * first + n_rays <= P, P < 2^40 and height x width < 2^31.  ctx may be NULL (stand-alone op). */
int knerf_draw_ray_batch(knerf_ctx* ctx, void* stream, const float* images, const float* c2w, int n_views, int height, int width,
                         int channels, float focal, float near_plane, float far_plane, int n_samples, uint64_t seed,
                         uint64_t epoch, uint64_t first, int n_rays, const float* noise, uint64_t noise_stream, float* o, float* d,
                         float* t, float* target, int64_t* index);

/* ---- Ray models for forward-facing scenes.  Extension, no reference counterpart (NDC rays and samples linear in disparity as in the
 * original NeRF release's LLFF configuration).  The two entry points below are knerf_generate_rays and knerf_draw_ray_batch with a ray
 * model: the same arguments, the same pixel order, the same Philox counters; the plain entry points and their kernels are untouched.
 *   ndc = 0, spacing = KNERF_SPACING_LINEAR: the plain rays and sample positions, bit for bit (model NULL means this).
 *   spacing = KNERF_SPACING_DISPARITY (pinhole rays only; near_plane > 0): with s = the plain stratified sample drawn on [0, 1],
 *     t = 1 / ((1 - s) / near_plane + s / far_plane): linear in 1 / t, monotone in s, so t stays sorted.
 *   ndc = 1: the pinhole ray (o, d) of a camera that looks along -z is mapped to normalised device coordinates with the near plane at
 *     distance n = ndc_near: the origin is moved onto the plane, s = -(n + o_z) / d_z, o <- o + s d; then
 *       o' = (-(2f/W) o_x/o_z, -(2f/H) o_y/o_z, 1 + 2n/o_z)
 *       d' = (-(2f/W) (d_x/d_z - o_x/o_z), -(2f/H) (d_y/d_z - o_y/o_z), -2n/o_z)
 *     Written are o' and the UNIT direction d' / L, L = |d'|, and t = s L with s the plain stratified sample drawn on
 *     [near_plane, far_plane], which must lie inside [0, 1]: o'_z = -1 and (o' + L d'/L)_z = +1, so t in [0, L] runs from the near
 *     plane to infinity and the deltas of compositing are Euclidean lengths in NDC space.  Rays parallel to the image plane
 *     (d_z = 0) have no NDC image; a forward-facing capture has none.
 * KNERF_ERR_INVALID, before any launch, on: what the plain entry points refuse; ndc or spacing outside their values; ndc_near <= 0 or
 * not finite; disparity spacing with near_plane <= 0; disparity spacing together with ndc; ndc with [near_plane, far_plane] outside
 * [0, 1]. */
enum { KNERF_SPACING_LINEAR = 0, KNERF_SPACING_DISPARITY = 1 };
typedef struct knerf_ray_model {
    int32_t ndc;                 /* 0 / 1 */
    int32_t spacing;             /* KNERF_SPACING_* */
    float ndc_near;              /* > 0; read only when ndc = 1 */
} knerf_ray_model;
int knerf_generate_rays_ext(knerf_ctx* ctx, void* stream, const float* c2w, const float* noise, uint64_t seed,
                            uint64_t stream_id, int batch, int height, int width, int n_samples, float focal,
                            float near_plane, float far_plane, float* o, float* d, float* t, const knerf_ray_model* model);
int knerf_draw_ray_batch_ext(knerf_ctx* ctx, void* stream, const float* images, const float* c2w, int n_views, int height, int width,
                             int channels, float focal, float near_plane, float far_plane, int n_samples, uint64_t seed,
                             uint64_t epoch, uint64_t first, int n_rays, const float* noise, uint64_t noise_stream, float* o, float* d,
                             float* t, float* target, int64_t* index, const knerf_ray_model* model);

/* ---- Camera models: full intrinsics, lens distortion, fisheye.  Extension, no reference counterpart (the conventions of OpenCV's
 * calib3d documentation, which COLMAP and nerfstudio / instant-ngp transforms.json files follow).  The two ray entry points below are
 * knerf_generate_rays_ext and knerf_draw_ray_batch_ext with a camera: the same arguments in the same order, the same pixel order,
 * the same Philox counters, `focal` replaced by (intrinsics, n_cameras, camera); every other entry point and kernel is untouched.
 *   intrinsics: DEVICE float [n_cameras, 12] = fx, fy, cx, cy, c0..c5, 0, 0
 *     OPENCV:  c = k1, k2, p1, p2, k3, 0        FISHEYE (equidistant): c = k1, k2, k3, k4, 0, 0
 *   n_cameras: 1 (one camera shared by every view) or the number of views of the call (row v for view v).
 * The ray of pixel (x, y) under a row: distorted normalised coordinates, image y pointing down,
 *     xn = ((float)x + pixel_offset - cx) / fx,  yn = ((float)y + pixel_offset - cy) / fy
 *   PINHOLE: (xu, yu) = (xn, yn).
 *   OPENCV: (xu, yu) solves distort(xu, yu) = (xn, yn), where with r^2 = x^2 + y^2 and rad = 1 + k1 r^2 + k2 r^4 + k3 r^6
 *     distort(x, y) = (x rad + 2 p1 x y + p2 (r^2 + 2 x^2),  y rad + p1 (r^2 + 2 y^2) + 2 p2 x y)
 *     by 2-D Newton with the analytic Jacobian from (xn, yn): exactly 8 iterations, no data-dependent exit.
 *   FISHEYE: theta solves theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = theta_d = hypot(xn, yn) by 1-D Newton from
 *     theta_d, 8 iterations; camera vector (sin theta xn/theta_d, -sin theta yn/theta_d, -cos theta), (0, 0, -1) at theta_d = 0:
 *     valid past 90 degrees.
 *   PINHOLE and OPENCV: camera vector (xu, -yu, -1).  Every model: rotated by c2w, normalised, origin = the translation column, with
 *   the operations of the plain kernels: PINHOLE with fx = fy = focal, cx = W * 0.5f, cy = H * 0.5f, pixel_offset = 0 writes the
 *   bits of knerf_generate_rays / knerf_draw_ray_batch (of the _ext entry points under a ray model).
 * The ray model is accepted as before (NULL: plain).  Sample positions do not depend on the camera, so disparity spacing works with
 * every camera; ndc = 1 applies the NDC map to the camera's ray with the scales -2 fx / W, -2 fy / H of row 0 and needs n_cameras = 1
 * and a model other than FISHEYE.
 * KNERF_ERR_INVALID, before any launch, on: what the _ext entry points refuse; a NULL camera or intrinsics pointer; model outside
 * KNERF_CAMERA_*; n_cameras outside {1, views}; pixel_offset not finite; ndc with FISHEYE or with n_cameras > 1.
 * NOT checked: the values of the table, which live on the device (no entry point here waits for it).  fx, fy > 0, finite values and a
 * lens that does not fold inside the image are the caller's to establish before the upload (keras_nerf_amd/data/cameras.py
 * CameraModel.check_invertible does): Newton on a folding lens converges to whatever root is near, or not at all. */
enum { KNERF_CAMERA_PINHOLE = 0, KNERF_CAMERA_OPENCV = 1, KNERF_CAMERA_FISHEYE = 2 };
typedef struct knerf_camera_model {
    int32_t model;               /* KNERF_CAMERA_*: one model per launch */
    float pixel_offset;          /* added to the integer pixel coordinates: 0 = pixel corners (the plain camera), 0.5 = centres */
} knerf_camera_model;
int knerf_generate_rays_cam(knerf_ctx* ctx, void* stream, const float* c2w, const float* noise, uint64_t seed,
                            uint64_t stream_id, int batch, int height, int width, int n_samples, const float* intrinsics,
                            int n_cameras, const knerf_camera_model* camera, float near_plane, float far_plane, float* o, float* d,
                            float* t, const knerf_ray_model* model);
int knerf_draw_ray_batch_cam(knerf_ctx* ctx, void* stream, const float* images, const float* c2w, int n_views, int height, int width,
                             int channels, const float* intrinsics, int n_cameras, const knerf_camera_model* camera,
                             float near_plane, float far_plane, int n_samples, uint64_t seed, uint64_t epoch, uint64_t first,
                             int n_rays, const float* noise, uint64_t noise_stream, float* o, float* d, float* t, float* target,
                             int64_t* index, const knerf_ray_model* model);
/* The forward map of the same cameras, one lane per point, no iteration, no context: points [n,3] (device) seen from view[i] (int32
 * [n]; NULL: view 0) with poses c2w [V,4,4] and the intrinsics row of that view (n_cameras = 1: row 0; else n_cameras = V).  With
 * p = R^T (x - t) the point in the camera's frame: depth [n] = -p_z; pixels [n,2] in the coordinates the ray kernels take -- the ray
 * of pixel (x, y) projects to (x, y); valid [n] (uint8) = depth > 0 for PINHOLE / OPENCV, and for FISHEYE: the point is not the camera
 * centre and theta < pi.  Values of view outside [0, V) are the caller's to exclude (V is not passed).  KNERF_ERR_INVALID on a NULL
 * pointer other than view, n = 0, n_cameras < 1, model out of range, pixel_offset not finite.  The error text is read with
 * knerf_last_error(NULL). */
int knerf_project_points(void* stream, const float* points, const int32_t* view, const float* c2w, const float* intrinsics,
                         int n_cameras, const knerf_camera_model* camera, uint64_t n, float* pixels, float* depth, uint8_t* valid);

/* ---- NeRFUtils as stand-alone ops (no context needed; the train/render path fuses the same arithmetic) ----
 * positional_encoding (utils.py:176-186): x [n_rows,3] -> out [n_rows, 3+6L].
 * composite = render_image_depth_chunk (utils.py:16-58): raw [R,S,4] = (r,g,b,sigma), t [R,S] -> image [R,3], depth [R]
 *   or NULL, weights [R,S] or NULL.
 * inverse_cdf = fine_hierarchical_sampling_chunk (utils.py:60-97) with u injected: mid_points [R,n_mid],
 *   weights [R,n_weights], u [R,n_samples] -> out [R,n_samples] (unsorted); 1 <= n_weights <= 4096, n_mid >= 1 and unrelated to it. */
int knerf_positional_encoding(void* stream, const float* x, long long n_rows, int L, float* out);
/* ray(t) = o + t d (utils.py:193-194): o, d [R,3], t [R,S] -> out [R,S,3] */
int knerf_ray_points(void* stream, const float* o, const float* d, const float* t, int n_rays, int n_samples, float* out);
/* the two image metrics NeRF.update_and_return_metrics logs (nerf.py:306-330; tf.image.psnr / tf.image.ssim defaults):
 * a, b [n_images, H, W, C] device; sums [n_images][2] = {sum of the SSIM terms over the (H-10)(W-10) VALID windows and C
 * channels, sum of squared differences}: ssim = sums[0] / ((H-10)(W-10)C), psnr = -10 log10(sums[1] / (HWC)). */
int knerf_image_metrics(void* stream, const float* a, const float* b, int n_images, int height, int width, int channels,
                        float* sums);
/* NeRF.update_and_return_metrics (nerf.py:306-330) without a host round trip: the six tf.keras.metrics.Mean objects as device
 * state [6][2] doubles = {total, count} in the order coarse_loss, coarse_psnr, coarse_ssim, fine_loss, fine_psnr, fine_ssim.
 * sums_coarse / sums_fine = knerf_image_metrics(images, coarse images) / (images, fine images) [n_images][2]; loss [2] = the
 * step's coarse and fine loss (device), or NULL for test_step's whole-image mean squared error (nerf.py:484-487) taken from
 * the same sums.  PSNR and SSIM add one value per image, the losses one per step, as Keras' Mean does. */
int knerf_metrics_update(void* stream, const float* sums_coarse, const float* sums_fine, const float* loss, int n_images,
                         int height, int width, int channels, double* state);
int knerf_composite(void* stream, const float* raw, const float* t, int n_rays, int n_samples, int white_background /* bit 0: white background, bit 1: no clip (utils.py:99-134) */,
                    float* image, float* depth, float* weights);
int knerf_inverse_cdf(void* stream, const float* mid_points, const float* weights, const float* u, int n_rays, int n_mid,
                      int n_weights, int n_samples, int oob_clamp, float* out);

/* Per-kernel timing with HIP events recorded on the caller's stream around every launch (bench.py's roofline leg).
 * Classes: 0 mlp_fwd coarse, 1 mlp_fwd fine, 2 composite, 3 sample_fine, 4 mlp_bwd coarse, 5 mlp_bwd fine,
 * 6 wgrad coarse, 7 wgrad fine, 8 adam+repack.  read() synchronises the device, returns summed milliseconds and launch
 * counts since enable/the previous read (n >= 9). */
int knerf_profile_enable(knerf_ctx* ctx, int on);
int knerf_profile_read(knerf_ctx* ctx, double* total_ms, int64_t* launches, int n);

/* ---- The trained field and its surface.  Extension, no reference counterpart (the original NeRF release's mesh-extraction
 * notebook evaluates the fine network on a dense grid; the reference ships none of this). ---- */
/* knerf_query_points -- extension, no reference counterpart.  The MLP `net` at n points: xyz [n,3]; dirs NULL (zero direction),
 * one shared [3] (dir_per_point 0) or [n,3] (dir_per_point 1).  Outputs (any may be NULL, not all): raw [n,4] = (rgb after sigmoid,
 * sigma after relu), sigma [n], rgb [n,3].  Fused shapes run one fused kernel (csrc/query.hip: the render path's encoding, trunk
 * and head, bit for bit); other shapes the positional-encoding op and the general-shape MLP in chunks of about 1 GB of workspace. */
int knerf_query_points(knerf_ctx* ctx, void* stream, int net, const float* xyz, const float* dirs, int dir_per_point, uint64_t n,
                       float* raw, float* sigma, float* rgb);
/* knerf_query_grid -- extension, no reference counterpart.  The same at every point of a [R0,R1,R2] grid (C order, z fastest;
 * n = R0 R1 R2): point (i,j,k) lies at lo + idx * step per axis, step = (hi - lo) / (R - 1) in fp32, the coordinate computed as
 * __fadd_rn(lo, __fmul_rn((float)idx, step)).  resolution, lo, hi: HOST [3] (R >= 2, hi > lo); dir: device [3] or NULL. */
int knerf_query_grid(knerf_ctx* ctx, void* stream, int net, const int32_t* resolution, const float* lo, const float* hi,
                     const float* dir, float* raw, float* sigma, float* rgb);
/* knerf_marching_cubes -- extension, no reference counterpart.  Context-free.  Iso-surface {sigma = threshold} of a device fp32 grid
 * [rx,ry,rz] placed as in knerf_query_grid (lo, hi HOST [3]); inside means sigma > threshold.  Indexed mesh: one vertex per crossed
 * grid edge, ordered by edge id (3 * point + axis); faces by cube, then table order (csrc/mesh_table.h); wound so that normals point
 * outward (toward lower density); normals = -grad sigma (central differences, one-sided at the border) interpolated along the edge,
 * normalised.  Three calls on one caller workspace:
 *   1. workspace NULL: *workspace_bytes = the size needed (rx ry rz <= 2^28);
 *   2. vertices, faces, normals all NULL: classification and scans; counts[0] = V, counts[1] = F (host; synchronises `stream`);
 *   3. the same workspace, grid and threshold: writes vertices [V,3], faces [F,3] (int32), normals [V,3] (each may be NULL).
 * Non-finite samples stay local: NaN is never > threshold (outside), +inf always is (inside), and the faces follow from that alone.
 * What the vertices on such a sample's six grid edges hold, and the normals whose gradient stencil (the six neighbours of an edge's
 * two ends) contains it, is unspecified; every other vertex and normal has the bits it has on the grid without that sample. */
int knerf_marching_cubes(void* stream, const float* grid, int rx, int ry, int rz, const float* lo, const float* hi, float threshold,
                         void* workspace, size_t* workspace_bytes, int64_t* counts, float* vertices, int32_t* faces, float* normals);

/* ---- Empty-space skipping for rendering.  Extension, no reference counterpart (occupancy grids as in Instant-NGP and Plenoxels). ----
 * Each net may carry one occupancy grid: cells[0] x cells[1] x cells[2] bits over the box [lo, hi].  With a grid attached to net n,
 * every RENDER pass of n runs the MLP only on samples whose cell is occupied (the coarse pass uses the coarse grid, the fine pass the
 * fine grid); every other sample gets raw = (0, 0, 0, 0): sigma = 0, alpha = 0, compositing weight exactly 0.  Compositing, the sampler
 * and the outputs work as before; the fine sampler takes the coarse weights that come out of this, so t_fine may differ from the dense
 * render.  A sample that is evaluated gets the bits the dense render (and knerf_query_points) gives it.
 *   Applies to:     knerf_render_chunk, knerf_render_batch; and, while option "occupancy_train" is 1, knerf_train_chunk and
 *                   knerf_train_batch.
 *   Never applies:  knerf_forward_chunk, knerf_query_points, knerf_query_grid; nor training while "occupancy_train" is 0 (the default).
 * Cell lookup of sample p = __fadd_rn(o, __fmul_rn(d, t)) (the render path's two roundings), per axis:
 *   u = __fmul_rn(__fsub_rn(p, lo), scale), scale = fp32(cells / (hi - lo)) computed in double on the host; i = floor(u).
 *   Outside the box: u < 0, i >= cells or u NaN on any axis; then the `outside` policy decides (occupied, or empty).
 *   Inside: bit (i cy + j) cz + k, i.e. bit b % 32 of little-endian uint32 word b / 32.
 * Fused shapes compact the live samples (an ordered scan) and run the fused MLP on that list only; the general-shape path
 * (shapes without fused kernels, KNERF_FLAG_FORCE_GENERIC) runs its MLP over every sample and zeroes the dead ones: the same outputs
 * without the speed-up.  The compaction runs under the net's forward profile class (knerf_profile_read classes 0 / 1).
 * Training behind a grid ("occupancy_train" = 1): every train pass of net n treats the samples in n's empty cells exactly as a render
 * does: raw = (0, 0, 0, 0) and the MLP is not evaluated there.  Their raw is a constant, so no gradient reaches the MLP from them; loss
 * and gradients are those of this masked field.  Fused shapes run the training forward, dgrad and weight gradients on the compacted
 * list of live samples (in 32-sample tiles that may straddle rays); the general-shape path runs densely, zeroes raw and dL/draw at the
 * dead samples and gives the same results without the speed-up.  With every cell occupied and "deterministic" on, losses, images and
 * gradients are bit-identical to training without a grid.  knerf_occupancy_train_stats counts these passes.
 * The grid is the caller's: training does not update it (knerf_occupancy_decay_max and knerf_occupancy_from_grid build the next one from
 * the field on the device; the Python package's OccupancyGridUpdater does so during fit). */
/* knerf_set_occupancy -- extension, no reference counterpart.  bits: DEVICE uint32 [ceil(cx cy cz / 32)], copied into a buffer the
 * context owns (on `stream`); NULL detaches the net's grid.  cells, lo, hi: HOST [3]; 1 <= cells <= 1024 and finite hi > lo per axis.
 * outside_empty: 0 = a sample outside the box is occupied, 1 = empty.  KNERF_ERR_INVALID on bad arguments and on a
 * KNERF_FLAG_ENCODED_WIDTHS context. */
int knerf_set_occupancy(knerf_ctx* ctx, void* stream, int net, const uint32_t* bits, const int32_t* cells, const float* lo, const float* hi,
                        int outside_empty);
/* knerf_occupancy_from_grid -- extension, no reference counterpart.  Context-free.  sigma: DEVICE fp32 lattice [rx,ry,rz] (e.g.
 * knerf_query_grid on [lo, hi]; 2 <= r <= 1025), so the grid has (rx-1) x (ry-1) x (rz-1) cells.  A cell is occupied if any of its 8
 * corners has sigma > threshold; then the occupied set is dilated by `dilation` cells (0..8, Chebyshev distance).  A heuristic: density
 * between lattice points can be missed, the dilation is the margin.  bits: DEVICE uint32 [ceil(cells / 32)] (padding bits 0). */
int knerf_occupancy_from_grid(void* stream, const float* sigma, int rx, int ry, int rz, float threshold, int dilation, uint32_t* bits);
/* knerf_occupancy_stats -- extension, no reference counterpart.  Per net since the last reset: live[n] = samples of render passes whose
 * MLP output is kept (occupied), total[n] = samples those passes considered (passes without a grid are not counted).
 * Synchronises `stream`. */
int knerf_occupancy_stats(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset);
/* knerf_occupancy_train_stats -- extension, no reference counterpart.  As knerf_occupancy_stats, for the TRAIN passes that ran behind a
 * grid ("occupancy_train" = 1): live[n] = samples whose MLP was evaluated, total[n] = samples those passes considered.  Render passes
 * are not counted here, train passes not in knerf_occupancy_stats.  Synchronises `stream`. */
int knerf_occupancy_train_stats(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset);
/* knerf_occupancy_decay_max -- extension, no reference counterpart (Instant-NGP's density EMA).  Context-free.  state, sigma: DEVICE fp32
 * [n]; state[i] = max(decay * state[i], sigma[i]) (one rounding for the product), on `stream`.  Needs 0 <= decay <= 1. */
int knerf_occupancy_decay_max(void* stream, float* state, const float* sigma, uint64_t n, float decay);
/* ---- Early ray termination for rendering.  Extension, no reference counterpart (as in Instant-NGP and most volume renderers). ----
 * With option "termination_threshold" eps > 0, every render pass (coarse and fine) of knerf_render_chunk / knerf_render_batch works in
 * segments: segment k of a ray is samples [k L, min((k+1) L, S)), L = option "termination_segment" (a segment longer than the pass is
 * the whole pass).  Segment 0 is evaluated as without the option (behind the grid, if one is attached).
 *   Transmittance: T = 1 in front of segment 0; after each segment T <- T * x_i for each of its samples in ascending order, one fp32
 *   product each, x_i = 1 - alpha_i + 1e-10, alpha_i = 1 - exp(-sigma_i delta_i), delta_i = t_{i+1} - t_i (the last 1e-10): the
 *   arithmetic of compositing, on the raw the pass has produced so far (0 at dead samples: x = 1 exactly).
 *   Cut: every sample of a later segment whose ray has T < fp32(eps) in front of that segment is TERMINATED: raw = (0, 0, 0, 0) and the
 *   MLP does not run on it.  A sample's MLP runs iff it is occupied (when a grid is attached) and not terminated.
 * Compositing, the sampler and the outputs work as before; the fine sampler takes the coarse weights that come out of this.  So:
 * terminated samples are a suffix of each ray that starts at a segment boundary; every sample in front of the cut has the bits of the
 * render without termination (dense, or grid-only with a grid); per ray the image moves by at most T_cut < eps per channel (with a
 * white background too: it moves by the change of sum w) and the depth by at most eps * t_max, up to fp32 summation order.
 *   Applies to:     knerf_render_chunk, knerf_render_batch.
 *   Never applies:  training, knerf_forward_chunk, knerf_query_points, knerf_query_grid (whatever eps is).
 * Fused shapes run one round per segment without host synchronisation: fold, cut, grid and an ordered compaction of the segment's live
 * samples, then the fused MLP on that list only (under the net's forward profile class).  Workspace, only while eps > 0: about 4 L + 8
 * bytes per ray.  The general-shape path runs its dense forward, then zeroes the terminated samples with the same rule: the same
 * outputs without the speed-up.  knerf_termination_stats counts these passes; knerf_occupancy_stats keeps counting the grid's verdict
 * on every sample. */
/* knerf_termination_stats -- extension, no reference counterpart.  Per net since the last reset: live[n] = samples of render passes with
 * eps > 0 whose MLP output is kept (occupied and not terminated; the fused path evaluates only those), total[n] = all samples of those
 * passes.  Synchronises `stream`. */
int knerf_termination_stats(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset);

/* ---- The baked field: a voxel grid with spherical-harmonic colour, rendered without the MLP.  Extension, no reference counterpart
 * (as PlenOctrees, SNeRG and Plenoxels bake a trained NeRF).  All three entry points are context-free; every pointer is a DEVICE
 * pointer unless it says HOST.
 * Lattice [Rx,Ry,Rz] (C order, z fastest; 2 <= R <= 1025 per axis) placed over [lo, hi] as in knerf_query_grid.  One RECORD per lattice
 * point, records in lattice order:
 *   bytes 0..3: fp32 sigma (the net's density after ReLU; the baker stores every value <= its threshold as 0);
 *   then 3 K halfs, K = (sh_degree + 1)^2, sh_degree 0..3, ordered [k][c] (coefficient k of colour channel c);
 *   zero padding to a multiple of 16 bytes: 16 / 32 / 64 / 112 bytes per record for degree 0 / 1 / 2 / 3.
 * Colour seen along the unit vector u: clamp(sum_k c_k Y_k(u), 0, 1), Y_k the orthonormal real spherical harmonics, k = l (l + 1) + m,
 * without the Condon-Shortley phase (Y_0 = 1 / (2 sqrt(pi)), Y_1..3 = sqrt(3 / (4 pi)) (y, z, x), ...: csrc/baked.hip sh_eval).
 * points x record bytes must stay below 2^40 (KNERF_ERR_INVALID otherwise); every element offset is computed in 64 bits. */
/* knerf_baked_project -- extension, no reference counterpart.  One direction of the least-squares SH fit, for i < n, k < n_coeff, c < 3:
 *   comp NULL:  acc[i][k][c] = fma(fit[k][j], rgb[i][c], acc[i][k][c]), one fused multiply-add per element;
 *   otherwise:  a compensated sum: acc takes the rounded sum, comp [n, n_coeff, 3] collects the rounding errors of the product (by fma)
 *               and of the sum (two-sum), both exact in fp32, so acc + comp carries the sum of all directions to about one rounding
 *               whatever the partial sums were (the plain form loses up to n_dirs x 2^-24 x the largest partial sum).
 * rgb [n,3], fit [n_coeff, n_dirs] (the pseudo-inverse of the basis at the fit directions), acc [n, n_coeff, 3], all fp32.
 * KNERF_ERR_INVALID: a NULL rgb, fit or acc, n_coeff not in {1, 4, 9, 16}, n_dirs < 1, j outside [0, n_dirs), acc of 2^40 bytes or more. */
int knerf_baked_project(void* stream, const float* rgb, const float* fit, int n_coeff, int n_dirs, int j, uint64_t n, float* acc,
                        float* comp);
/* knerf_baked_pack -- extension, no reference counterpart.  Writes n whole records: record p = index[i] (int64 [n], every value in
 * [0, n_points); index NULL: p = i and n = n_points) gets sigma[p] (sigma: fp32 [n_points], the whole lattice) and acc[i] [K,3] fp32
 * (comp not NULL: fp32(acc[i] + comp[i]), knerf_baked_project's pair) rounded to fp16 (nearest even).  Records not named keep their
 * bytes (the baker starts from zeros).
 * KNERF_ERR_INVALID: a NULL sigma, acc or records, sh_degree outside 0..3, n > n_points, index NULL with n != n_points,
 * n_points x record bytes >= 2^40. */
int knerf_baked_pack(void* stream, const float* sigma, const float* acc, const float* comp, const int64_t* index, uint64_t n,
                     uint64_t n_points, int sh_degree, void* records);
/* knerf_baked_render -- extension, no reference counterpart.  Volume rendering of n_rays rays through a baked field.
 * field: HOST struct; records as above; bits: the occupancy bitfield of the (Rx-1)(Ry-1)(Rz-1) cells in the layout of
 * knerf_set_occupancy (bit set = some corner has sigma > 0), needed only with KNERF_BAKED_SKIP_EMPTY.
 * origins, directions [n_rays,3]; near, far [n_rays] or NULL (then near_all / far_all hold for every ray).  t is in units of |d|:
 * directions need not be unit vectors.  Per ray, in fp32 unless said otherwise:
 *   S = ceil((far - near) / step) evaluated in double (at most 2^23), samples i = 0..S-1 at t_i = near + (i + 0.5) step,
 *   p = __fadd_rn(o, __fmul_rn(d, t_i)).  Sample positions do not depend on the box; the ray-box intersection only narrows the range of
 *   i that is visited (an axis with d = 0 is inside for all t if lo <= o <= hi, else the ray misses).
 *   u = __fmul_rn(__fsub_rn(p, lo), scale), scale = fp32(cells / (hi - lo)) computed in double (knerf_set_occupancy's lookup); a sample
 *   with u < 0, u > cells or u NaN on any axis is outside: sigma = 0.  Otherwise cell = min(floor(u), cells - 1) (a sample on the upper
 *   face belongs to the last cell), sigma and the coefficients are interpolated trilinearly with weights from u - cell.
 *   alpha = 1 - expf(-sigma step |d|), w = T alpha, image += w colour(d / |d|), depth += w t_i, opacity += w, T <- T (1 - alpha),
 *   strictly in ascending i, T = 1 at the start.  termination = eps > 0: the ray stops once T < eps.
 *   KNERF_BAKED_WHITE_BACKGROUND: image += 1 - opacity at the end.  The image is clipped to [0, 1].
 * KNERF_BAKED_SKIP_EMPTY: samples in cells whose bit is 0 are not fetched.  With bits as described their trilinear sigma is exactly 0,
 * so alpha = w = 0 and T is unchanged: outputs with and without the flag are bit-identical.
 * Lanes per ray (bits 8..11 of flags): 0 = the library's choice, 1 = one ray per lane, 2 (degree 1) / 4 (degree 2 and 3) = a group of
 * lanes reads each record as one contiguous fetch and adds its channel sums across lanes; the choices differ in summation order only.
 * image [n_rays,3], depth [n_rays], opacity [n_rays]: each may be NULL.  stats: int64 [2] or NULL; [0] += samples whose 8 corners
 * were fetched, [1] += sum of S over the rays (one atomic pair per wave).
 * KNERF_ERR_INVALID, before any launch: NULL field, records, origins or directions; no output and no stats; sh_degree outside 0..3; a
 * resolution outside 2..1025; lo / hi not finite or hi <= lo; points x record bytes >= 2^40; step <= 0 or not finite; termination
 * outside [0, 1); unknown flag bits, a lane count the degree does not have, SKIP_EMPTY without bits; n_rays >= 2^36. */
enum { KNERF_BAKED_WHITE_BACKGROUND = 1, KNERF_BAKED_SKIP_EMPTY = 2, KNERF_BAKED_LANES_SHIFT = 8, KNERF_BAKED_LANES_MASK = 0xF00 };
typedef struct knerf_baked_field {
    const void* records;         /* DEVICE */
    const uint32_t* bits;        /* DEVICE, may be NULL without KNERF_BAKED_SKIP_EMPTY */
    int32_t resolution[3];       /* lattice points per axis */
    int32_t sh_degree;           /* 0..3 */
    float lo[3], hi[3];
} knerf_baked_field;
int knerf_baked_render(void* stream, const knerf_baked_field* field, const float* origins, const float* directions, const float* near,
                       const float* far, float near_all, float far_all, uint64_t n_rays, float step, float termination, int flags,
                       float* image, float* depth, float* opacity, int64_t* stats);

/* ---- Optimising a baked field against ray batches.  Extension, no reference counterpart (as PlenOctrees and Plenoxels optimise their
 * grids after conversion).  Two context-free launches; csrc/baked_train.hip, tests/baked_train_reference.py restates them in fp64.
 * knerf_baked_train: HOST struct.  field: the records (knerf_baked_train_apply WRITES them) and, as bits, the SUPPORT bitfield: the
 * cells that are ever fetched, fixed while the field is optimised, a superset of the cells with a non-zero sigma; never NULL here.
 * slot_of: int32 [points], the slot of every lattice point that is a corner of a support cell, -1 elsewhere.  grad: fp32
 * [n_slots][1 + 3 K] gradient rows in the column order of a record: sigma, then [k][c].  1 <= n_slots <= points. */
typedef struct knerf_baked_train {
    knerf_baked_field field;
    const int32_t* slot_of;      /* DEVICE */
    float* grad;                 /* DEVICE */
    uint64_t n_slots;
} knerf_baked_train;
/* knerf_baked_train_rays -- extension, no reference counterpart.  ADDS to grad the gradient of
 *   L = (1 / 3 N) sum_rays sum_c (out_c - target_c)^2,  N = n_norm (0: n_rays),  out = the image of knerf_baked_render
 * marched with KNERF_BAKED_SKIP_EMPTY over the support bits (always, whether the flag is given or not), same step, termination,
 * white-background flag and lane variants (flags as knerf_baked_render).  target [n_rays,3].  Each ray is marched twice in the launch:
 * first the render kernel's arithmetic sample for sample (C = sum w col, O = sum w), then again to scatter.  Both clamps pass the
 * gradient on the closed interval [0, 1]; the cut of a terminated ray is held fixed; coefficients are differentiated at their stored
 * fp16 values.  With g_c = 2 (out_c - target_c) / (3 N) [0 <= C_c + bg (1 - O) <= 1], bg = 1 with the white background else 0,
 * A_j = sum_c g_c (col_jc - bg), delta = step |d| and tau_n the trilinear weights of sample j's 8 corners n:
 *   grad[n][sigma] += tau_n delta (T_{j+1} A_j - sum_{i>j} w_i A_i)        (no division by 1 - alpha)
 *   grad[n][k][c]  += tau_n Y_k g_c w_j [0 <= r_jc <= 1]                   r the colour before its clamp
 * by fp32 atomic adds: the sums depend on arrival order in their last bits.  sq_err: [n_rays] or NULL; the ray's
 * sum_c (out_c - target_c)^2, a plain store.
 * KNERF_ERR_INVALID, before any launch: NULL train, records, bits, slot_of, grad, origins, directions or target; n_slots outside
 * [1, points]; n_norm >= 2^36; and every argument error of knerf_baked_render. */
int knerf_baked_train_rays(void* stream, const knerf_baked_train* train, const float* origins, const float* directions, const float* near,
                           const float* far, float near_all, float far_all, const float* target, uint64_t n_rays, uint64_t n_norm,
                           float step, float termination, int flags, float* sq_err);
/* knerf_baked_train_rays_ext -- extension, no reference counterpart.  knerf_baked_train_rays under the objective record of the train
 * step (knerf_objective above; its `nets` field is IGNORED here: a grid has no coarse / fine pair): the robust losses and the two
 * regularisers of a ray's weights, for a grid.  Per ray, over the samples the march fetches, in march order, up to and including the
 * sample behind which a termination cut falls: w_j, O = sum w_j, C, pre = C + bg (1 - O), out = clip(pre, 0, 1), d_c = out_c - target_c as
 * above; delta = step |d|, the length of every fetched sample's interval; m_j = (i_j - i_first) delta, i_j the sample's index on the ray
 * and i_first that of the ray's first fetched sample (D is shift-invariant; samples that are skipped never enter).  With N = n_norm
 * (0: n_rays) the launch ADDS to grad the gradient of
 *   L = 1 / (3 N) sum_rays sum_c rho(d_c) + (distortion / N) sum_rays D + (opacity_entropy / N) sum_rays H
 *   rho: the four kinds of KNERF_LOSS_* as defined above; g_c = rho'(d_c) / (3 N) [0 <= pre_c <= 1]
 *   D = sum_i sum_j w_i w_j |m_i - m_j| + delta / 3 sum_i w_i^2, evaluated with the exclusive prefixes W_k = sum_{j<k} w_j,
 *       M_k = sum_{j<k} w_j m_j and MT = sum w m:   D = 2 sum_k w_k (m_k W_k - M_k) + delta / 3 sum_k w_k^2,
 *       dD/dw_k = 2 (2 m_k W_k - 2 M_k + MT - m_k O) + 2/3 delta w_k,   sum_k w_k dD/dw_k = 2 D
 *   H = -a ln a - (1 - a) ln(1 - a), a = clamp(O, 1e-4, 1 - 1e-4);  dH/dw_k = ln((1 - a) / a) where 1e-4 <= O <= 1 - 1e-4, else 0
 *   A_j = sum_c g_c (col_jc - bg) + (distortion / N) dD/dw_j + (opacity_entropy / N) dH/dw_j
 *   grad[n][sigma] += tau_n delta (T_{j+1} A_j - sum_{i>j} w_i A_i),   the coefficient columns as above with the new g_c.
 * The regularisers are functions of the weights alone: they pass neither clamp, so a ray whose g is 0 on every channel still adds their
 * gradient.  The termination cut stays fixed; t, step and the sample positions carry no gradient.  The photometric share of the sum over
 * later samples is the plain kernel's (exactly 0 at a ray's last sample); the regularisers' share is their total (wd 2 D + we dH O) minus
 * a running prefix and carries the total's rounding.
 * objective == NULL, or KNERF_LOSS_MSE with both weights 0: the call IS knerf_baked_train_rays -- the same kernel, the same bits -- and
 * `terms` is left untouched.  Otherwise the extended kernel runs (one per degree, lane variant and storage; kind and weights are run-time
 * values) and terms, fp32 [n_rays][4] or NULL, receives per ray (sum_c rho(d_c), sum_c d_c^2, D, H) by plain stores; a ray without a
 * fetched sample stores D = 0 and H = H(1e-4).  sq_err as above.
 * KNERF_ERR_INVALID, before any launch: everything knerf_baked_train_rays refuses; an unknown loss_kind; huber_delta <= 0 or not finite
 * under KNERF_LOSS_HUBER; a weight that is negative or not finite. */
int knerf_baked_train_rays_ext(void* stream, const knerf_baked_train* train, const float* origins, const float* directions,
                               const float* near, const float* far, float near_all, float far_all, const float* target, uint64_t n_rays,
                               uint64_t n_norm, float step, float termination, int flags, float* sq_err,
                               const knerf_objective* objective, float* terms);
/* knerf_baked_train_rays_rgba -- extension, no reference counterpart.  knerf_baked_train_rays_ext against RGBA photographs: a background
 * per ray, the target recomposited over it with the photograph's alpha, and a loss between the ray's opacity and that alpha (what grid
 * methods do against cut-out images: a floater in front of an empty pixel then differs from the background and has a gradient). */
typedef struct knerf_baked_rgba {
    const float* background;    /* DEVICE [n_rays,3], or NULL: 1 with KNERF_BAKED_WHITE_BACKGROUND, else 0, on every channel */
    const float* alpha;         /* DEVICE [n_rays], or NULL: the target is used as it is (every alpha then reads as 1) */
    float stored_background;    /* 0 or 1: what the target's rgb is already composited over */
    float opacity;              /* lambda_o >= 0; > 0 needs alpha */
} knerf_baked_rgba;
/* C, O, w_j, delta, N, rho, D, H as in knerf_baked_train_rays_ext; all fp32 without contraction, in the order written.  Per ray:
 *   b_c = background[ray][c], or the flag's value;   pre_c = C_c + b_c (1 - O),   out_c = clip(pre_c, 0, 1)
 *   tgt_c = target_c + (1 - alpha) (b_c - stored_background) with alpha, else target_c: a target stored as alpha rgb + (1 - alpha) B0
 *       becomes the photograph over b; it is not clipped
 *   d_c = out_c - tgt_c,   g_c = rho'(d_c) / (3 N) [0 <= pre_c <= 1]
 *   L = 1 / (3 N) sum rho(d_c) + (distortion / N) sum D + (opacity_entropy / N) sum H + (opacity / N) sum (O - alpha)^2
 *   A_j = sum_c g_c (col_jc - b_c) + r_j,   r_j = (distortion / N) dD/dw_j + (opacity_entropy / N) dH/dw + (opacity / N) 2 (O - alpha)
 *   later samples: sum_c g_c ((C_c - P_c) - b_c (O - P_O)) + (total - running prefix),
 *       total = (distortion / N) 2 D + ((opacity_entropy / N) dH/dw + (opacity / N) 2 (O - alpha)) O
 * The opacity term passes neither clamp: a ray whose g is 0 on every channel still adds its gradient once it fetched a sample; a ray
 * without a fetched sample adds none.  With b = 1 the expression 1 (1 - O) has the bits of the white flag's 1 - O, with b = 0 the sum
 * C + 0 has the bits of C: a background array of ones (zeros) without alpha and weight gives the bits of the flag's _ext call.
 * terms, fp32 [n_rays][5] or NULL: the four of _ext, then (O - alpha)^2 (alpha = 1 without an alpha array).
 * rgba == NULL, or background == NULL && alpha == NULL && opacity == 0: the call IS knerf_baked_train_rays_ext (the same launch, the same
 * bits; terms is then [n_rays][4], and under a plain objective untouched).  Otherwise the rgba kernel runs, also under a plain objective.
 * KNERF_ERR_INVALID, before any launch: everything knerf_baked_train_rays_ext refuses; stored_background other than 0 or 1; opacity
 * negative or not finite; opacity > 0 without alpha.  Every lane variant of _ext exists for the rgba kernel too.  The device values of
 * background and alpha are not read back. */
int knerf_baked_train_rays_rgba(void* stream, const knerf_baked_train* train, const float* origins, const float* directions,
                                const float* near, const float* far, float near_all, float far_all, const float* target, uint64_t n_rays,
                                uint64_t n_norm, float step, float termination, int flags, float* sq_err,
                                const knerf_objective* objective, float* terms, const knerf_baked_rgba* rgba);
/* knerf_baked_train_rays_depth -- extension, no reference counterpart.  knerf_baked_train_rays_rgba with depth supervision: a measured
 * depth per ray (a structure-from-motion point seen through the pixel, an RGB-D capture, another model's depth map) and a squared loss
 * between it and the ray's expected depth, the one term of the objective that says WHERE along the ray the weight sits. */
typedef struct knerf_baked_depth {
    const float* target;   /* DEVICE [n_rays], ray-parameter units: what knerf_baked_render writes as depth */
    const float* weight;   /* DEVICE [n_rays] >= 0, or NULL: every ray 1 */
    float depth;           /* lambda_z >= 0 */
} knerf_baked_depth;
/* Everything of knerf_baked_train_rays_rgba, and all fp32 without contraction, in the order written.  Per ray:
 *   t_j = near + (i_j + 0.5) step, the ray parameter of the fetched sample i_j, as the march forms it
 *   Z = sum_j w_j t_j, accumulated in march order as Z = Z + w t over the fetched samples up to and including the one behind which a
 *       termination cut falls: the bits of knerf_baked_render's depth for the same ray, step, termination, lane variant and
 *       KNERF_BAKED_SKIP_EMPTY over the support bits
 *   z* = target[ray],   c = weight[ray], or 1
 *   L gains (depth / N) sum_rays c (Z - z*)^2
 *   zeta = (depth / N) 2 c (Z - z*);   r_j gains zeta t_j (the depth share of A_j),   total gains zeta Z
 * A ray with c == 0 has a depth term and a zeta of exactly 0 whatever z* holds, NaN included (a select, not a product: sparse depth
 * maps are mostly empty).  t, step and the cut carry no gradient.  The term passes neither clamp: a ray whose g is 0 on every channel
 * still adds its gradient once it fetched a sample and c > 0; a ray without a fetched sample has Z = 0, stores c z*^2 and adds none.
 * terms, fp32 [n_rays][6] or NULL: the five of _rgba, then c (Z - z*)^2.
 * depth == NULL, or depth->depth == 0: the call IS knerf_baked_train_rays_rgba (the same launch, the same bits, terms with that route's
 * stride, and that route's own fall-through to _ext and the plain call).  Otherwise the depth kernel runs, also under a plain objective
 * and without an rgba record: its rgba fields then read as that contract's defaults (the flag's background, every alpha 1, opacity 0).
 * KNERF_ERR_INVALID, before any launch: everything knerf_baked_train_rays_rgba refuses; depth->depth negative or not finite;
 * depth->depth > 0 with target == NULL.  Every lane variant of _rgba exists for the depth kernel too.  The device values of target and
 * weight are not read back. */
int knerf_baked_train_rays_depth(void* stream, const knerf_baked_train* train, const float* origins, const float* directions,
                                 const float* near, const float* far, float near_all, float far_all, const float* target, uint64_t n_rays,
                                 uint64_t n_norm, float step, float termination, int flags, float* sq_err,
                                 const knerf_objective* objective, float* terms, const knerf_baked_rgba* rgba,
                                 const knerf_baked_depth* depth);
/* knerf_baked_train_apply -- extension, no reference counterpart.  One Adam step over all slots and the records rewritten.
 * point_of: int32 [n_slots], the lattice point of a slot (the inverse of slot_of); sigma_trainable: uint8 [n_slots]; master, m, v:
 * fp32 [n_slots][1 + 3 K] like grad.  Per column, Keras form: m += (g - m)(1 - beta_1), v += (g g - v)(1 - beta_2),
 * w -= rate m / (sqrt(v) + epsilon), rate = rate_sigma for the sigma column and rate_sh for the others: the caller's
 * learning_rate sqrt(1 - beta_2^t) / (1 - beta_1^t), computed in double from its own step count t.  The sigma column is updated only
 * where sigma_trainable is set (elsewhere w, m, v keep their values) and projected: w <- max(w, 0).  Then the slot's record is
 * rewritten (fp32 sigma, coefficients rounded to fp16 to nearest even, zero padding) and the gradient row is zeroed.
 * KNERF_ERR_INVALID: as above, a NULL point_of, sigma_trainable, master, m or v, a rate that is not finite, a beta outside [0, 1),
 * epsilon <= 0. */
int knerf_baked_train_apply(void* stream, const knerf_baked_train* train, const int32_t* point_of, const uint8_t* sigma_trainable,
                            float* master, float* m, float* v, float rate_sigma, float rate_sh, float beta_1, float beta_2, float epsilon);

/* ---- Growing a baked field: a total-variation regulariser for the optimiser above and resampling onto another lattice (coarse to
 * fine).  Extension, no reference counterpart (Plenoxels regularises and refines its grid in this way).  Two context-free launches;
 * csrc/baked_grow.hip, tests/baked_grow_reference.py restates them in NumPy. */
/* knerf_baked_train_tv -- extension, no reference counterpart.  ADDS to grad the gradient of
 *   R = weight_sigma sum_p tv_sigma(p) + weight_sh sum_p sum_{q != sigma} tv_q(p),    p over the slots, q over the columns of a row,
 *   tv_q(p) = sqrtf(D_x^2 + D_y^2 + D_z^2 + epsilon),   D_a q(p) = v_q(p + e_a) - v_q(p) if p + e_a lies in the lattice AND has a slot,
 *   otherwise 0;  v_q(p) = master[slot_of[p]][q], the fp32 master value (master, point_of: as knerf_baked_train_apply).  Points without
 * a slot never enter, whatever their record holds.  The sigma column of a slot that is not trainable takes part as a value (its
 * master is 0) and its gradient is written like any other: knerf_baked_train_apply ignores it.  The caller passes the weights PER
 * TERM (the Python package: lambda_sigma / n_slots and lambda_sh / (3 K n_slots), formed in double).
 * The gradient is a gather: per (slot, column), in fp32,
 *   g = w [ -sum_a D_a(p) / tv(p) + sum_a D_a(p - e_a) / tv(p - e_a) ],    the second sum over the predecessors that have a slot,
 * formed in registers and added to grad with ONE fp32 add and no atomics: grad_after = fp32(grad_before + g) exactly, and two calls
 * from the same state give the same bits.  A weight of exactly 0 leaves the columns of its group untouched, bit for bit.
 * tv_out: fp32 [n_slots][2] or NULL; [p][0] = tv_sigma(p), [p][1] = sum_{q != sigma} tv_q(p) (summed in double in column order, rounded
 * once), unweighted, plain stores.  With both weights 0 and tv_out NULL nothing is launched.
 * KNERF_ERR_INVALID, before any launch: NULL train, point_of or master; epsilon <= 0 or not finite; a weight that is negative or not
 * finite; every struct error of knerf_baked_train_apply. */
int knerf_baked_train_tv(void* stream, const knerf_baked_train* train, const int32_t* point_of, const float* master, float weight_sigma,
                         float weight_sh, float epsilon, float* tv_out);
/* knerf_baked_resample -- extension, no reference counterpart.  The records of the field src on another lattice dst_resolution (HOST
 * [3], 2 <= R' <= 1025 per axis, points x record bytes < 2^40) over the same [lo, hi], same sh_degree.  New index i of an axis with R old
 * and R' new points:  u = (double)i (R - 1) / (R' - 1) in double,  cell = min(floor(u), R - 2),  f = (float)(u - cell).  Every
 * value is interpolated trilinearly from the 8 old points of the cell, along z, then y, then x, each step
 *   lerp(a, b, f) = __fadd_rn(__fmul_rn(a, __fsub_rn(1, f)), __fmul_rn(b, f))       (no fused multiply-add)
 * so that f = 0 returns a and f = 1 returns b exactly.  sigma is interpolated in fp32 and a result <= sigma_threshold is stored as
 * exactly 0; coefficients go fp16 -> fp32 -> interpolate -> fp16 (nearest even); the padding is written as zeros.  src->bits is not
 * read.  Consequences: an old cell with sigma = 0 at its 8 corners gives sigma = 0 at every new point inside it, so
 * knerf_occupancy_from_grid(sigma', 0, 0) yields bits that are exact for skipping; with R' = 2 R - 1 every old point reappears with
 * its values unchanged as numbers; the first and last point of an axis are kept for every R'.
 * KNERF_ERR_INVALID, before any launch: NULL src, records, dst_resolution or dst_records; sh_degree outside 0..3; a resolution (old
 * or new) outside 2..1025; lo / hi not finite or hi <= lo; either table of 2^40 bytes or more; sigma_threshold negative or not
 * finite; dst_records overlapping the source records. */
int knerf_baked_resample(void* stream, const knerf_baked_field* src, const int32_t dst_resolution[3], float sigma_threshold,
                         void* dst_records);

/* ---- The baked field as sparse bricks.  Extension, no reference counterpart (PlenOctrees, SNeRG's macroblock atlas and Plenoxels store
 * only the occupied part of their grids behind a coarse index).  One context-free launch; csrc/baked_bricks.hip,
 * tests/baked_bricks_reference.py restates the format in NumPy.
 * The lattice [Rx,Ry,Rz] of a baked field is cut into bricks of b^3 lattice points, b = 1 << brick_log2 = 4 or 8.  Point (x, y, z)
 * lies in brick (x >> brick_log2, y >> brick_log2, z >> brick_log2) of the brick grid B_a = ceil(R_a / b), at place
 * ((x & (b-1)) b + (y & (b-1))) b + (z & (b-1)) inside it.  A brick is STORED iff it holds at least one touched point (a corner of a
 * cell whose occupancy bit is set); stored bricks are numbered 0..n_bricks-1 in ascending C order of the brick index.
 *   brick_of: int32 [Bx][By][Bz], the slot of a stored brick, -1 for an absent one;
 *   records:  [n_bricks][b^3] records in the layout above; a stored brick is a verbatim copy of the dense records of all its points
 *             (untouched ones included), points of an edge brick outside the lattice are all-zero records;
 *   bits:     the occupancy bitfield of the dense field, unchanged.
 * A point of an absent brick reads as an all-zero record.  A brick_of value < 0 or >= n_bricks is treated as absent by the kernel: a
 * damaged table never becomes an out-of-range read.  n_bricks >= 1: a field without an occupied cell carries one all-zero brick 0 that
 * no brick_of entry names.  n_bricks x b^3 x record bytes must stay below 2^40; every element offset is computed in 64 bits. */
typedef struct knerf_baked_bricks {
    const void* records;         /* DEVICE */
    const int32_t* brick_of;     /* DEVICE */
    const uint32_t* bits;        /* DEVICE, may be NULL without KNERF_BAKED_SKIP_EMPTY */
    int32_t resolution[3];       /* lattice points per axis */
    int32_t sh_degree;           /* 0..3 */
    float lo[3], hi[3];
    int32_t brick_log2;          /* 2 or 3 */
    uint64_t n_bricks;
} knerf_baked_bricks;
/* knerf_baked_render_bricks -- extension, no reference counterpart.  knerf_baked_render through the brick table: the same march (sample
 * positions, cell lookup, corner order, fused multiply-adds, lane variants, batches of occupancy words, termination, stats), every
 * argument behind `field` as there.  Only the address of a corner's record differs, so for a brick field that holds the dense field's
 * stored bricks all outputs and stats are bit-identical to knerf_baked_render's: an absent brick holds no corner of an occupied cell,
 * the dense sigma there is 0, and a sample whose sigma is 0 adds +0 whatever its colour is.
 * KNERF_ERR_INVALID, before any launch: everything knerf_baked_render refuses; a NULL brick_of; brick_log2 outside {2, 3}; n_bricks = 0
 * or above Bx By Bz; n_bricks x b^3 x record bytes >= 2^40. */
int knerf_baked_render_bricks(void* stream, const knerf_baked_bricks* field, const float* origins, const float* directions,
                              const float* near, const float* far, float near_all, float far_all, uint64_t n_rays, float step,
                              float termination, int flags, float* image, float* depth, float* opacity, int64_t* stats);

/* ---- Optimising a brick field as it is.  Extension, no reference counterpart.  The two launches of "Optimising a baked field" above on
 * the brick layout, so that no table of the dense lattice's size exists at any point; csrc/baked_bricks_train.hip.  The NumPy reference of
 * a brick optimiser over a field F is tests/baked_train_reference.py on the dense arrays of F (absent bricks read as zero);
 * tests/baked_bricks_train_reference.py restates the brick set, the flags and the row order.
 * knerf_baked_bricks_train: HOST struct.  field: the optimiser's OWN brick set -- every brick that holds a corner of a SUPPORT cell,
 * numbered as knerf_baked_bricks numbers stored bricks; records: knerf_baked_bricks_train_apply WRITES them; bits: the SUPPORT bitfield
 * (as knerf_baked_train: the cells that are ever fetched, fixed while the field is optimised), never NULL here.  There is no slot table:
 * grad, and master, m, v below, hold one row per STORED RECORD, fp32 [n_bricks b^3][1 + 3 K] in the column order of a record (sigma, then
 * [k][c]), and a row's index is the record's index: slot b^3 + place.  Rows of records that are no corner of a support cell (and of places
 * past the lattice) exist and stay zero. */
typedef struct knerf_baked_bricks_train {
    knerf_baked_bricks field;
    float* grad;                 /* DEVICE */
} knerf_baked_bricks_train;
/* knerf_baked_bricks_train_rays -- extension, no reference counterpart.  knerf_baked_train_rays through the brick table: the same two
 * marches, loss, gradient formulas, atomic adds and sq_err, every argument behind `train` as there.  Only a corner's address differs
 * (formed as in knerf_baked_render_bricks).  A corner whose brick_of entry is < 0 or >= n_bricks reads as a zero record and NOTHING is
 * added for it: a damaged table never becomes an out-of-range read or write.  For a brick set that holds every corner of every support
 * cell the sums a row receives are those of knerf_baked_train_rays on the dense field, addend for addend.
 * Lane variants: those of knerf_baked_train_rays (all of them build without scratch; 0 in the flags picks the library's default).
 * KNERF_ERR_INVALID, before any launch: everything knerf_baked_render_bricks refuses of its field, NULL bits or grad, every argument error
 * of knerf_baked_train_rays, a lane count the degree does not have among them. */
int knerf_baked_bricks_train_rays(void* stream, const knerf_baked_bricks_train* train, const float* origins, const float* directions,
                                  const float* near, const float* far, float near_all, float far_all, const float* target,
                                  uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* sq_err);
/* knerf_baked_bricks_train_rays_ext -- extension, no reference counterpart.  knerf_baked_train_rays_ext through the brick table: the same
 * objective, marches, per-ray terms and refusals (`nets` ignored; objective NULL or plain: the call IS knerf_baked_bricks_train_rays and
 * `terms` is left untouched), a corner's address formed as in knerf_baked_bricks_train_rays.  For a brick set that holds every corner of
 * every support cell, gradient addends and terms are those of knerf_baked_train_rays_ext on the dense field, bit for bit.
 * KNERF_ERR_INVALID, before any launch: everything knerf_baked_bricks_train_rays and knerf_baked_train_rays_ext refuse. */
int knerf_baked_bricks_train_rays_ext(void* stream, const knerf_baked_bricks_train* train, const float* origins, const float* directions,
                                      const float* near, const float* far, float near_all, float far_all, const float* target,
                                      uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* sq_err,
                                      const knerf_objective* objective, float* terms);
/* knerf_baked_bricks_train_rays_rgba -- extension, no reference counterpart.  knerf_baked_train_rays_rgba through the brick table: the
 * same record, arithmetic, terms [n_rays][5] and refusals (rgba NULL or empty: the call IS knerf_baked_bricks_train_rays_ext); for a
 * brick set that holds every corner of every support cell the addends are those of the dense call, bit for bit. */
int knerf_baked_bricks_train_rays_rgba(void* stream, const knerf_baked_bricks_train* train, const float* origins, const float* directions,
                                       const float* near, const float* far, float near_all, float far_all, const float* target,
                                       uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* sq_err,
                                       const knerf_objective* objective, float* terms, const knerf_baked_rgba* rgba);
/* knerf_baked_bricks_train_rays_depth -- extension, no reference counterpart.  knerf_baked_train_rays_depth through the brick table: the
 * same record, arithmetic, terms [n_rays][6] and refusals (depth NULL or weight 0: the call IS knerf_baked_bricks_train_rays_rgba); Z has
 * the bits of knerf_baked_render_bricks' depth, and for a brick set that holds every corner of every support cell the addends are those
 * of the dense call, bit for bit. */
int knerf_baked_bricks_train_rays_depth(void* stream, const knerf_baked_bricks_train* train, const float* origins, const float* directions,
                                        const float* near, const float* far, float near_all, float far_all, const float* target,
                                        uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* sq_err,
                                        const knerf_objective* objective, float* terms, const knerf_baked_rgba* rgba,
                                        const knerf_baked_depth* depth);
/* knerf_baked_bricks_train_apply -- extension, no reference counterpart.  knerf_baked_train_apply over the stored records: the same Adam
 * step, projection, record rewrite (fp32 sigma, coefficients to fp16 to nearest even, zero padding) and zeroing of the gradient row.
 * flags: uint8 [n_bricks b^3]; bit 0: the record is a slot (a corner of a support cell), bit 1: its sigma is trainable.  A record without
 * bit 0 is skipped entirely: its record, master, m, v and grad keep their bytes.  master, m, v: fp32 rows like grad.
 * KNERF_ERR_INVALID: as above, a NULL flags, master, m or v, a rate that is not finite, a beta outside [0, 1), epsilon <= 0. */
int knerf_baked_bricks_train_apply(void* stream, const knerf_baked_bricks_train* train, const uint8_t* flags, float* master, float* m,
                                   float* v, float rate_sigma, float rate_sh, float beta_1, float beta_2, float epsilon);

/* ---- Growing a brick field as it is.  Extension, no reference counterpart.  "Growing a baked field" above on the brick layout, so that
 * a field is resampled, regularised and pruned without a table of the dense lattice's size; csrc/baked_bricks_grow.hip,
 * tests/baked_bricks_grow_reference.py restates it in NumPy.  The arithmetic of a lattice point is one text for both storages
 * (csrc/baked_grow_common.h): each launch gives the bits of its dense counterpart on the dense arrays of the field (absent bricks read as
 * zero records).  Every table lookup is range-checked before an address is formed; every element offset is computed in 64 bits. */
/* knerf_baked_resample_bricks_sigma -- extension, no reference counterpart.  The first pass of resampling a brick field: dst_sigma, fp32
 * [R'x][R'y][R'z] (DEVICE), the sigma knerf_baked_resample stores at every point of the lattice dst_resolution (HOST [3]) from the dense
 * arrays of src: the same placement (u in double, cell, f), the same lerp along z, then y, then x, a result <= sigma_threshold stored as
 * exactly 0.  One lane per new point; a source corner whose brick_of entry is < 0 or >= n_bricks reads as a zero record.  src->bits is not
 * read.  From dst_sigma the caller forms the new occupancy bits (knerf_occupancy_from_grid(sigma', 0, 0)) and from them the new brick table.
 * KNERF_ERR_INVALID, before any launch: NULL src, dst_resolution or dst_sigma; everything knerf_baked_render_bricks refuses of its field;
 * every argument error of knerf_baked_resample (a new resolution outside 2..1025, a new table of 2^40 bytes or more, sigma_threshold
 * negative or not finite). */
int knerf_baked_resample_bricks_sigma(void* stream, const knerf_baked_bricks* src, const int32_t dst_resolution[3], float sigma_threshold,
                                      float* dst_sigma);
/* knerf_baked_resample_bricks -- extension, no reference counterpart.  The second pass: the records of the destination's stored bricks.
 * dst: HOST struct with the destination's lattice, box, degree, brick size, brick table and n_bricks; dst->records and dst->bits are not
 * read (dst_records is what is written).  dst_keys: int32 [n_bricks'] (DEVICE), the linear index in the destination's brick grid of every
 * stored destination brick, ascending (the inverse of dst->brick_of).  dst_records: [n_bricks'][b'^3] records, one lane per (record,
 * 16-byte chunk).  A place past the lattice, and every record of a brick whose key lies outside the brick grid, is written as zeros, so
 * the caller may pass uninitialised memory.  Every other record is what knerf_baked_resample writes for that lattice point from the dense
 * arrays of src: fp32 sigma with the threshold, coefficients fp16 -> fp32 -> fp16 to nearest even, zero padding.  The source and
 * destination brick sizes may differ.
 * KNERF_ERR_INVALID, before any launch: NULL src, dst, dst_keys or dst_records; everything knerf_baked_render_bricks refuses of either
 * field (dst->records apart); a degree or a box that differs between the two; sigma_threshold negative or not finite; dst_records
 * overlapping the source records. */
int knerf_baked_resample_bricks(void* stream, const knerf_baked_bricks* src, const knerf_baked_bricks* dst, const int32_t* dst_keys,
                                float sigma_threshold, void* dst_records);
/* knerf_baked_bricks_train_tv -- extension, no reference counterpart.  knerf_baked_train_tv on the rows of knerf_baked_bricks_train: ADDS
 * to grad the gradient of the same R with v_q(p) = master[record of p][q].  A point takes part iff it lies in the lattice, its brick is
 * stored and its flag has bit 0 (flags: as knerf_baked_bricks_train_apply); for a train-brick set that is the dense optimiser's slot set.
 * keys: int32 [n_bricks] (DEVICE), the linear brick-grid index of every stored brick, ascending (the inverse of brick_of): a record
 * learns its lattice point from it.  The records of a brick whose key lies outside the brick grid take no part.  A record without bit 0
 * keeps its gradient row and gets tv_out = (0, 0).  g of a record's column is formed in registers by knerf_baked_train_tv's formula in
 * its order of operations and added to grad with ONE fp32 add, no atomics: the rows get the bits knerf_baked_train_tv gives the same master
 * and gradient values, and two calls from the same state give the same bits.  A weight of exactly 0 leaves the columns of its group
 * untouched.  tv_out: fp32 [n_bricks b^3][2] or NULL, as there.  With both weights 0 and tv_out NULL nothing is launched.
 * KNERF_ERR_INVALID, before any launch: NULL train, keys, flags or master; epsilon <= 0 or not finite; a weight that is negative or not
 * finite; every struct error of knerf_baked_bricks_train_apply. */
int knerf_baked_bricks_train_tv(void* stream, const knerf_baked_bricks_train* train, const int32_t* keys, const uint8_t* flags,
                                const float* master, float weight_sigma, float weight_sh, float epsilon, float* tv_out);

/* ---- Refining camera poses against a baked field.  Extension, no reference counterpart (BARF, NeRF-- and the current toolkits optimise
 * their cameras with the field).  Three context-free launches; csrc/baked_pose.hip, tests/baked_pose_reference.py restates them in fp64,
 * DESIGN.md 2.24 has the derivation.  The MLP path has no input gradient; NDC rays are not covered (the pose does not enter them as
 * o = t, d = R cam). */
/* knerf_baked_ray_gradients -- extension, no reference counterpart.  The gradient of the objective of knerf_baked_train_rays,
 *   L = (1 / 3 N) sum_rays sum_c (out_c - target_c)^2,  N = n_norm (0: n_rays),
 * with respect to every ray's origin and direction.  field->bits is the support that is marched (never NULL here); rays, near / far,
 * target, n_norm, step, termination and flags are those of knerf_baked_train_rays, and so are the forward march, both clamps, the
 * white background, the termination cut and dsig_j = dL/dsigma_j, dr_jc = dL/dr_jc (total minus prefix).  With t_j the sample's ray
 * parameter, u = d / |d|, delta = step |d|, fr the fractions of the sample in its cell, scale_a = (R_a - 1) / (hi_a - lo_a):
 *   G_j            = scale * (dsig_j grad_fr sigma + sum_c dr_jc grad_fr r_c)      grad_fr: the trilinear weights' derivative, the 8 corners
 *                                                                                 with one factor replaced by +-1; r_c of a corner = sum_k Y_k(u) coef_kc
 *   grad_origin    = sum_j G_j
 *   grad_direction = sum_j t_j G_j + (sum_j dsig_j sigma_j) (step / delta) u + (1 / |d|) (I - u u^T) sum_j sum_c dr_jc sum_k cf_jkc grad Y_k(u)
 * grad Y_k: the gradient of the polynomials of sh_eval as written (the projection removes the choice of extension off the sphere).
 * The discontinuities carry no gradient (a sample entering or leaving the box, the window or a cell's support, the termination cut,
 * the clamps): the convention of knerf_baked_train_rays.  |d| = 0: both gradients are zero.
 * grad_origin, grad_direction: fp32 [n_rays,3], WRITTEN for every ray (zeros where nothing contributes), each ray's by its own lane
 * group, once: no atomics, no scratch buffer, the same bits on every launch.  sq_err: [n_rays] or NULL, as knerf_baked_train_rays.
 * Lane variants: those of knerf_baked_train_rays (they differ in summation order only).
 * KNERF_ERR_INVALID, before any launch: NULL field, records, bits, origins, directions, target, grad_origin or grad_direction; and every
 * argument error of knerf_baked_train_rays. */
int knerf_baked_ray_gradients(void* stream, const knerf_baked_field* field, const float* origins, const float* directions,
                              const float* near, const float* far, float near_all, float far_all, const float* target, uint64_t n_rays,
                              uint64_t n_norm, float step, float termination, int flags, float* grad_origin, float* grad_direction,
                              float* sq_err);
/* knerf_baked_ray_gradients_bricks -- extension, no reference counterpart.  knerf_baked_ray_gradients through the brick table: the same
 * kernel, only a corner's address differs (formed as in knerf_baked_render_bricks; a brick_of entry < 0 or >= n_bricks reads as a zero
 * record, never as an out-of-range address).  For a brick field that holds the dense field's stored bricks the outputs are
 * bit-identical to knerf_baked_ray_gradients' at the same lane variant.
 * KNERF_ERR_INVALID, before any launch: as above, and everything knerf_baked_render_bricks refuses of its field. */
int knerf_baked_ray_gradients_bricks(void* stream, const knerf_baked_bricks* field, const float* origins, const float* directions,
                                     const float* near, const float* far, float near_all, float far_all, const float* target,
                                     uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* grad_origin,
                                     float* grad_direction, float* sq_err);
/* knerf_pose_gradients -- extension, no reference counterpart.  Per-ray gradients summed to one rigid-motion gradient per camera:
 *   out[v][0..2] = sum_{view[i] = v} grad_origin[i]                        (tau)
 *   out[v][3..5] = sum_{view[i] = v} directions[i] x grad_direction[i]     (omega)
 * the derivative at 0 of R <- exp(omega^) R, t <- t + tau for rays o = t, d = R cam (normalised or not): it needs neither the
 * camera-space direction nor the focal length.  view: int32 [n_rays], the camera of every ray (the Python package divides the flat
 * pixel index of knerf_draw_ray_batch by the pixels per view); an index outside [0, n_views) is skipped.  out: DOUBLE [n_views][6],
 * written whole (a view without a ray gets zeros).  The sums are formed in double in a fixed order without atomics: two launches on
 * the same inputs give the same bits.
 * KNERF_ERR_INVALID, before any launch: a NULL pointer; n_rays >= 2^36; n_views >= 2^31. */
int knerf_pose_gradients(void* stream, const float* grad_origin, const float* grad_direction, const float* directions,
                         const int32_t* view, uint64_t n_rays, uint64_t n_views, double* out);

/* ---- The brick baked field with 8-bit SH coefficients.  Extension, no reference counterpart (PlenOctrees and SNeRG ship their SH
 * coefficients as 8-bit values with a scale).  Three context-free launches; csrc/baked_quant.hip, tests/baked_quant_reference.py restates
 * the format in NumPy, DESIGN.md 2.25 has the exactness argument.
 * SOURCE: any knerf_baked_bricks set: records [n_bricks][b^3], b = 4 or 8, degree 0..3, K = (degree + 1)^2 coefficients [k][c].
 * BANDS: coefficient k belongs to SH band l = floor(sqrt(k)).
 * EXPONENT: one exponent e per stored brick s and band l <= degree.  M = the maximum of |c| over all b^3 places of the brick, all k of
 *   band l and all three channels (untouched points and the zero places past the lattice included), the values read as their stored
 *   fp16 bits, a NaN counting as 0.  e = the smallest integer in [-24, 9] with 127 2^e >= M; if there is none, e = 9; M = 0 gives
 *   e = -24.  Stored as uint32 exponents[n_bricks]: byte l (bits 8l..8l+7) holds e as a two's-complement int8; bytes of bands above the
 *   degree are written 0 and are never trusted by a reader.
 * COEFFICIENT: q = clamp(rint(c 2^-e), -127, 127): the product is exact in fp32 and rounded to nearest even; NaN becomes 0; +-inf and
 *   magnitudes above 65024 saturate to +-127 at e = 9.  q is stored as a two's-complement int8.  Decoded value: dec = (float)q 2^e,
 *   exact in fp32 and exactly representable in fp16: 127 x 2^9 <= 65504, so decoding never overflows, and e >= -24, so every decoded
 *   value is a multiple of the fp16 subnormal spacing.  For |c| <= 65024: |c - dec| <= 2^(e-1), which for e > -24 is < M / 127.
 * RECORD: 8 / 16 / 32 / 64 bytes for degree 0 / 1 / 2 / 3.  Bytes 0..3: the fp32 sigma, copied bit for bit; byte 4 + 3 k + c: q[k][c];
 *   zero padding fills the rest and a reader never trusts it.  A zero record decodes to zeros, so absent bricks and places past the
 *   lattice behave as they do in knerf_baked_bricks.  brick_of, the occupancy bits, resolution, bounds, brick size are the source
 *   field's, unchanged (the quantised field may share the source's brick_of and bits): empty-space skipping stays bit-exact.
 * Consequences: quantising the dequantised records gives the quantised records and exponents back byte for byte; the dequantised
 * records are an ordinary knerf_baked_bricks set, and knerf_baked_render_qbricks with one ray per lane gives the bits of
 * knerf_baked_render_bricks with one ray per lane on them. */
typedef struct knerf_baked_qbricks {
    knerf_baked_bricks bricks;   /* bricks.records: the QUANTISED records, DEVICE */
    const uint32_t* exponents;   /* DEVICE, [n_bricks] */
} knerf_baked_qbricks;
/* knerf_baked_quantize_bricks -- extension, no reference counterpart.  Encodes the records of src: dst_exponents [n_bricks] and
 * dst_records [n_bricks][b^3] quantised records are WRITTEN whole (padding and unused exponent bytes as zeros).  One workgroup per stored
 * brick; the band maxima are order-independent, so two launches give the same bytes; no atomics, no host read.  src->brick_of and
 * src->bits are not read and may be NULL.
 * KNERF_ERR_INVALID, before any launch: NULL src, records, dst_records or dst_exponents; everything knerf_baked_render_bricks refuses of
 * its field (degree, brick_log2, resolution, bounds, n_bricks, n_bricks x b^3 x either record size >= 2^40); destination records or
 * exponents that overlap the source records or each other. */
int knerf_baked_quantize_bricks(void* stream, const knerf_baked_bricks* src, void* dst_records, uint32_t* dst_exponents);
/* knerf_baked_dequantize_bricks -- extension, no reference counterpart.  dst_records [n_bricks][b^3] ordinary brick records: the sigma
 * bits copied, the coefficients dec rounded to fp16 (exact), zero padding.  An exponent byte outside [-24, 9] is clamped into it.
 * KNERF_ERR_INVALID, before any launch: as above with NULL exponents; dst_records overlapping the source records or exponents. */
int knerf_baked_dequantize_bricks(void* stream, const knerf_baked_qbricks* src, void* dst_records);
/* knerf_baked_render_qbricks -- extension, no reference counterpart.  knerf_baked_render_bricks on the quantised records as they are:
 * the same march, every argument behind `field` as there.  Only the fetch differs: the record has the size above, the exponent word of a
 * corner's brick is read by slot, and every corner's coefficients are decoded to fp32 before they enter the trilinear sum (the 8 corners
 * may lie in 8 bricks with 8 exponents; the group variants multiply the corner's weight by 2^e instead, which is exact short of
 * underflow and gives fma the same exact product).  A brick_of value < 0 or >= n_bricks reads as a zero record; an exponent byte outside [-24, 9]
 * is clamped into it: a damaged table never becomes an out-of-range read or a value that is not finite.
 * Lanes per ray (bits 8..11 of flags): 0 = the library's choice, 1 = one ray per lane (every degree; the sums run in the order of
 * knerf_baked_render_bricks' one-ray-per-lane variant), 2 (degree 2) / 4 (degree 3) = every lane of a group reads one 16-byte chunk of a
 * record; the choices differ in summation order only.
 * KNERF_ERR_INVALID, before any launch: everything knerf_baked_render_bricks refuses; NULL exponents; a lane count the degree does not
 * have. */
int knerf_baked_render_qbricks(void* stream, const knerf_baked_qbricks* field, const float* origins, const float* directions,
                               const float* near, const float* far, float near_all, float far_all, uint64_t n_rays, float step,
                               float termination, int flags, float* image, float* depth, float* opacity, int64_t* stats);

/* ---- What a baked field holds at a point.  Extension, no reference counterpart (Plenoxels and PlenOctrees answer point queries on
 * their grids and export meshes from them).  csrc/baked_query.hip; tests/baked_query_reference.py restates the arithmetic in fp64.
 * knerf_baked_query / knerf_baked_query_bricks / knerf_baked_query_qbricks -- density, colour along a direction and the density's
 * gradient of a dense, a brick and an 8-bit brick field at n points.  The evaluation is knerf_baked_render's evaluation of one sample.
 * query: HOST struct.  The points are EITHER a list, points [n,3] (DEVICE), OR a grid (grid_resolution[3], grid_lo[3], grid_hi[3]: HOST,
 * all three given, points NULL and n ignored): then n = Rx Ry Rz and point idx = (i Ry + j) Rz + k (C order, z fastest) lies, per axis, at
 *   __fadd_rn(lo, __fmul_rn((float)idx_axis, step)), step = (hi - lo) / (R - 1) in fp32
 * as knerf_query_grid places it; no coordinate tensor exists.  The grid's box is independent of the field's box.
 * Per point p, in fp32:
 *   CELL.  Per axis u = __fmul_rn(__fsub_rn(p, lo), scale), scale = fp32(cells / (hi - lo)) computed in double, cells = R - 1 (the
 *   lookup of knerf_baked_render).  The point is inside iff 0 <= u <= cells on every axis; a NaN coordinate is outside.  Outside: sigma,
 *   rgb and gradient are exactly 0.  Inside: cell = min(floor(u), cells - 1) (a point on the upper face belongs to the last cell),
 *   f = u - cell.
 *   DENSITY.  Corners cn = 0..7 with x = bit 2, y = bit 1, z = bit 0; weight w_cn = ((cn&4 ? fx : 1-fx) * (cn&2 ? fy : 1-fy)) *
 *   (cn&1 ? fz : 1-fz); sigma = the sum in ascending cn of fma(w_cn, sigma_cn, sum).  This is the sample of knerf_baked_render: a
 *   queried sigma is the sigma the march composites at that position.
 *   COLOUR (only where rgb is asked for).  Every coefficient is interpolated with the same weights in the same fma order; slots of a
 *   record that hold no coefficient count as 0 whatever their bits are.  colour_c = sum over k of fma(coeff[k][c], Y_k(d / |d|), sum),
 *   with one point per lane in ascending e = 3 k + c, clamped to [0, 1].  d is normalised as the render normalises it:
 *   |d| = sqrt(dx dx + dy dy + dz dz), d / |d| per component.  directions: NULL, one shared [3] (per_point = 0) or [n,3] (per_point =
 *   1), DEVICE.  A NULL direction, or one whose length is 0 or not finite (a NaN component included), gives the DC term alone:
 *   colour_c = clamp(Y_0 coeff[0][c]); the bands above 0 do not enter.
 *   GRADIENT (optional).  The exact gradient of the trilinear sigma inside the located cell, d sigma / d p: per axis a, with b < c the
 *   other two axes, scale_a * S_a, S_a = the sum over the four corner pairs (lower corner cn with the axis' bit clear, in ascending cn)
 *   of fma(w_b w_c, sigma_(cn | bit) - sigma_cn, sum), w_b and w_c the one-axis weights above (f or 1 - f), one final multiply by
 *   scale_a.  The trilinear sigma is not differentiable across cell faces: a point on a face gets the gradient of the cell picked above
 *   (the cell on its upper side; on the box's upper face the last cell).
 * Storage.  Bricks: a corner's record is found through brick_of as in knerf_baked_render_bricks (a value < 0 or >= n_bricks reads as a
 * zero record); dense and bricks of the same field give identical bits.  8-bit bricks: every corner's coefficients are decoded to fp32
 * before they enter the fma (an exponent byte outside [-24, 9] is clamped into it); with one point per lane the result has the bits of
 * knerf_baked_query_bricks with one point per lane on the dequantised records.
 * Lanes per point (bits 8..11 of flags, KNERF_BAKED_LANES_*): 0 = the library's choice, 1 = one point per lane, or the group of the
 * storage's renderer (dense, bricks: 2 at degree 1, 4 at degrees 2 and 3; 8-bit: 2 at degree 2, 4 at degree 3): a group reads each
 * corner record as one contiguous fetch of 16-byte chunks and adds its channel sums across lanes; the choices differ in the colour's
 * summation order only.  No other flag bit exists.
 * sigma [n], rgb [n,3], gradient [n,3] (DEVICE; in grid mode [Rx,Ry,Rz], [Rx,Ry,Rz,3]): each may be NULL, not all.  Without rgb only the
 * first word of each corner record is loaded (4 bytes, not the record), directions are not read and the lane choice has no effect;
 * the sigma and gradient bits are those of a call with rgb.
 * KNERF_ERR_INVALID, before any launch: a NULL field, records (brick_of, exponents) or query; everything knerf_baked_render (_bricks)
 * refuses of its field; no output; neither points nor a grid, or both; a grid given in part; a grid resolution < 2 or a grid of more
 * than 2^31 points; a grid box that is not finite, has hi <= lo or a step that is not finite; per_point outside {0, 1}; unknown flag
 * bits; a lane count the degree does not have; n >= 2^36.  n = 0 succeeds without a launch. */
typedef struct knerf_baked_query_spec {
    const float* points;             /* DEVICE [n,3], or NULL with a grid */
    uint64_t n;                      /* points in the list (ignored with a grid) */
    const int32_t* grid_resolution;  /* HOST [3], or NULL with a list */
    const float* grid_lo;            /* HOST [3] */
    const float* grid_hi;            /* HOST [3] */
    const float* directions;         /* DEVICE: NULL, [3] or [n,3] */
    int32_t per_point;               /* directions: 0 = one shared [3], 1 = [n,3] */
    int32_t flags;                   /* lanes per point in KNERF_BAKED_LANES_MASK */
    float* sigma;                    /* DEVICE [n] or NULL */
    float* rgb;                      /* DEVICE [n,3] or NULL */
    float* gradient;                 /* DEVICE [n,3] or NULL */
} knerf_baked_query_spec;
int knerf_baked_query(void* stream, const knerf_baked_field* field, const knerf_baked_query_spec* query);
int knerf_baked_query_bricks(void* stream, const knerf_baked_bricks* field, const knerf_baked_query_spec* query);
int knerf_baked_query_qbricks(void* stream, const knerf_baked_qbricks* field, const knerf_baked_query_spec* query);

/* Diagnostics (layout tables, workspace views, hardware-fact and bandwidth probes) are NOT part of this library: they are
 * declared in include/knerf_debug.h and built into libknerf_probe.so for tests/ and tools/ only. */

#ifdef __cplusplus
}
#endif
#endif /* KNERF_H */
