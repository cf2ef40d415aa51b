// optim_ext.h -- the opt-in extensions of the optimizer step (include/knerf.h knerf_set_optimizer): learning-rate schedules evaluated
// on the device, gradient clipping (by value, per-tensor norm, global norm of one net) and decoupled weight decay.  The plain step
// (optim.hip adam_kernel / step_status_kernel / step_set_kernel) is untouched; knerf_apply_adam launches the kernels declared here only
// while some extension is active.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/knerf.h"
#include "kernels.h"

namespace knerf {

constexpr int kOptMaxTensors = 256;      // 2 n_layers + 8 tensors per net (n_layers <= 64: 136); one thread each in clip_scale_kernel
constexpr int kOptItemElems = 4096;      // elements per workgroup of the sum-of-squares pass (a tensor is cut into items of at most this)

// what the single-thread kernels evaluate, by value in the kernel arguments.  lr(step) in double; beta1 / beta2 as knerf_config holds them.
struct SchedArgs {
    int kind, staircase, n_values;
    double lr, decay_steps, decay_rate, alpha, weight_decay;
    long long boundaries[KNERF_SCHEDULE_MAX_VALUES - 1];
    double values[KNERF_SCHEDULE_MAX_VALUES];
    float b1, b2;
};

struct AdamExtArgs {
    AdamArgs a;
    int clip;                    // KNERF_CLIP_* (0: none)
    float clip_value;            // KNERF_CLIP_VALUE: the bound, rounded once to fp32
    const float* scale;          // KNERF_CLIP_NORM: one factor per tensor of this net; KNERF_CLIP_GLOBAL_NORM: [0] the net's factor
    const int* tensor_off;       // KNERF_CLIP_NORM: n_tensors + 1 ascending offsets into the flat parameter vector
    int n_tensors;
    const float* decay;          // device: fp32(weight_decay * lr(step)) of this step, or null (no weight decay)
};
hipError_t launch_adam_ext(const AdamExtArgs& x, hipStream_t stream);

// End of a step / the step counter set from the host, as step_status_kernel / step_set_kernel, with the scheduled rate: lr_t and
// decay (may be null) are those of the NEXT step.  step < 0 in launch_step_set_ext keeps the device-side counter (knerf_set_optimizer).
hipError_t launch_step_status_ext(const int* flag, int* host_status, int* step_state, float* lr_t, float* decay, const SchedArgs& s, hipStream_t stream);
hipError_t launch_step_set_ext(int step, int* step_state, float* lr_t, float* decay, const SchedArgs& s, hipStream_t stream);

// Sum of squares of g = [coarse | fine] (n floats per net) in double, one workgroup per item (a slice [begin, end) of ONE tensor, the
// same items for both nets): partial [2][n_items].  No atomics: a fixed tree inside the workgroup.  Folds the finite check of
// check_finite_kernel in (*flag = 1 on any non-finite element; the items cover every element).
hipError_t launch_sumsq_partial(const float* g, int n, const int* item_begin, const int* item_end, int n_items, double* partial, int* flag, hipStream_t stream);
// Ordered second pass (one workgroup per net): the items of each tensor in ascending order, then -- for the global norm -- the
// tensors in ascending order; the factor in double, rounded once, exactly 1.0f where nothing is clipped.
// KNERF_CLIP_NORM: scale[net][t] = c / max(|g_t|, c); KNERF_CLIP_GLOBAL_NORM: scale[net][0] = min(1, c / |g|).  scale: [2][kOptMaxTensors].
hipError_t launch_clip_scale(const double* partial, int n_items, const int* tensor_item0, int n_tensors, int clip, double c, float* scale, hipStream_t stream);

}  // namespace knerf
