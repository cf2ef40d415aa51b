// optim_ext.hip -- learning-rate schedules, gradient clipping and decoupled weight decay around Keras-form Adam (optim_ext.h;
// include/knerf.h knerf_set_optimizer).  Restates tf.keras.optimizers.Adam(learning_rate=<schedule>, clipvalue / clipnorm /
// global_clipnorm, weight_decay) as the reference would get it from tf.keras.optimizers.get (keras_nerf/model/nerf/nerf.py:163-165):
//   lr(step)  step = optimizer steps APPLIED before this one (Keras evaluates the schedule at `iterations` before incrementing);
//   clip      on the gradient found in the accumulator, after the finite check, before the moments;
//   decay     w -= w * (weight_decay * lr(step))   -- the scheduled rate, not lr_t; before the Adam update of the same step;
//   Adam      as optim.hip adam_kernel, lr_t = lr(step) sqrt(1 - b2^t) / (1 - b1^t), t = step + 1.
// Everything that depends on the step count is evaluated ON THE DEVICE, in double, by the single-thread kernels behind each step, so
// a skipped (non-finite) step advances nothing and queued steps need no host round trip.
#include <hip/hip_runtime.h>

#include "optim_ext.h"

namespace knerf {

__global__ void adam_ext_kernel(AdamExtArgs x) {
    const AdamArgs& a = x.a;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    float g = a.g[i];
    a.g[i] = 0.f;                                   // also after a skipped step, as adam_kernel
    if (*a.nonfinite) return;
    if (x.clip == KNERF_CLIP_VALUE) {
        g = fminf(fmaxf(g, -x.clip_value), x.clip_value);
    } else if (x.clip == KNERF_CLIP_NORM) {
        int lo = 0, hi = x.n_tensors;               // the tensor t with tensor_off[t] <= i < tensor_off[t + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (x.tensor_off[mid] <= i) lo = mid; else hi = mid;
        }
        g = g * x.scale[lo];
    } else if (x.clip == KNERF_CLIP_GLOBAL_NORM) {
        g = g * x.scale[0];
    }
    float w = a.w[i];
    if (x.decay) w = w - w * *x.decay;
    float m = a.m[i], v = a.v[i];
    m = m + (g - m) * (1.f - a.b1);
    v = v + (g * g - v) * (1.f - a.b2);
    a.m[i] = m; a.v[i] = v;
    a.w[i] = w - *a.lr_t * m / (sqrtf(v) + a.eps);
}
hipError_t launch_adam_ext(const AdamExtArgs& x, hipStream_t stream) {
    hipLaunchKernelGGL(adam_ext_kernel, dim3((x.a.n + 255) / 256), dim3(256), 0, stream, x);
    return hipGetLastError();
}

// ---- the scheduled rate (one thread) --------------------------------------------------------------------------------------------
__device__ double scheduled_lr(const SchedArgs& s, int step) {
    const double x = (double)step;
    if (s.kind == KNERF_SCHEDULE_EXPONENTIAL) {
        double p = x / s.decay_steps;
        if (s.staircase) p = floor(p);
        return s.lr * pow(s.decay_rate, p);
    }
    if (s.kind == KNERF_SCHEDULE_COSINE) {
        const double c = x < s.decay_steps ? x : s.decay_steps;
        return s.lr * ((1.0 - s.alpha) * (0.5 * (1.0 + cos(3.14159265358979323846 * c / s.decay_steps))) + s.alpha);
    }
    if (s.kind == KNERF_SCHEDULE_PIECEWISE) {
        constexpr int M = KNERF_SCHEDULE_MAX_VALUES;
        double v = s.values[0];
        bool found = false;
#pragma unroll
        for (int i = 0; i < M; ++i) {               // values[i] for the first i with step <= boundaries[i], else the last value
            const bool hit = i >= s.n_values - 1 || (long long)step <= s.boundaries[i < M - 1 ? i : M - 2];
            if (!found && hit) { v = s.values[i]; found = true; }
        }
        return v;
    }
    return s.lr;
}
// lr_t in the operation order of optim.hip keras_lr_t (a constant schedule gives its bits); decay = fp32(weight_decay * lr(step))
__device__ void next_rates(const SchedArgs& s, int step, float* lr_t, float* decay) {
    const double lr = scheduled_lr(s, step);
    const int t = step + 1;
    *lr_t = (float)(lr * sqrt(1.0 - pow((double)s.b2, (double)t)) / (1.0 - pow((double)s.b1, (double)t)));
    if (decay) *decay = (float)(s.weight_decay * lr);
}
__global__ void step_status_ext_kernel(const int* flag, int* host_status, int* step_state, float* lr_t, float* decay, SchedArgs s) {
    if (*flag) {
        host_status[0] = host_status[0] + 1;
    } else {
        step_state[0] = step_state[0] + 1;
        next_rates(s, step_state[0], lr_t, decay);
    }
    host_status[1] = host_status[1] + 1;
    __threadfence_system();
}
hipError_t launch_step_status_ext(const int* flag, int* host_status, int* step_state, float* lr_t, float* decay, const SchedArgs& s, hipStream_t stream) {
    hipLaunchKernelGGL(step_status_ext_kernel, dim3(1), dim3(1), 0, stream, flag, host_status, step_state, lr_t, decay, s);
    return hipGetLastError();
}
__global__ void step_set_ext_kernel(int step, int* step_state, float* lr_t, float* decay, SchedArgs s) {
    if (step >= 0) step_state[0] = step;
    next_rates(s, step_state[0], lr_t, decay);
}
hipError_t launch_step_set_ext(int step, int* step_state, float* lr_t, float* decay, const SchedArgs& s, hipStream_t stream) {
    hipLaunchKernelGGL(step_set_ext_kernel, dim3(1), dim3(1), 0, stream, step, step_state, lr_t, decay, s);
    return hipGetLastError();
}

// ---- norms --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* g, int n, const int* item_begin, const int* item_end, int n_items,
                                                            double* partial, int* flag) {
    const int item = blockIdx.x, net = blockIdx.y;
    const float* gn = g + (size_t)net * n;
    const int end = item_end[item];
    double acc = 0.0;
    bool bad = false;
    for (int i = item_begin[item] + (int)threadIdx.x; i < end; i += 256) {
        const float x = gn[i];
        bad |= !__builtin_isfinite(x);
        acc += (double)x * (double)x;               // |x| <= 3.4e38: the square is finite in double, and so is any sum of 2^31 of them
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ double s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)net * n_items + item] = (s[0] + s[1]) + (s[2] + s[3]);
    if (bad) *flag = 1;
}
hipError_t launch_sumsq_partial(const float* g, int n, const int* item_begin, const int* item_end, int n_items, double* partial, int* flag, hipStream_t stream) {
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(n_items, 2), dim3(256), 0, stream, g, n, item_begin, item_end, n_items, partial, flag);
    return hipGetLastError();
}

__global__ __launch_bounds__(kOptMaxTensors) void clip_scale_kernel(const double* partial, int n_items, const int* tensor_item0, int n_tensors, int clip,
                                                                    double c, float* scale) {
    const int net = blockIdx.x, t = threadIdx.x;
    __shared__ double ssq[kOptMaxTensors];
    if (t < n_tensors) {
        double a = 0.0;
        for (int k = tensor_item0[t]; k < tensor_item0[t + 1]; ++k) a += partial[(size_t)net * n_items + k];
        ssq[t] = a;
        if (clip == KNERF_CLIP_NORM) {
            const double norm = sqrt(a);
            scale[net * kOptMaxTensors + t] = (float)(c / (norm > c ? norm : c));
        }
    }
    __syncthreads();
    if (clip == KNERF_CLIP_GLOBAL_NORM && t == 0) {
        double a = 0.0;
        for (int k = 0; k < n_tensors; ++k) a += ssq[k];
        const double norm = sqrt(a);
        scale[net * kOptMaxTensors] = norm > c ? (float)(c / norm) : 1.f;
    }
}
hipError_t launch_clip_scale(const double* partial, int n_items, const int* tensor_item0, int n_tensors, int clip, double c, float* scale, hipStream_t stream) {
    if (n_tensors > kOptMaxTensors) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_scale_kernel, dim3(2), dim3(kOptMaxTensors), 0, stream, partial, n_items, tensor_item0, n_tensors, clip, c, scale);
    return hipGetLastError();
}

}  // namespace knerf
