// composite_ext.h -- the opt-in extensions of the compositing kernel's objective (include/knerf.h knerf_set_objective): photometric
// terms other than the squared error and two per-ray regularisers, in csrc/composite_ext.hip.  Callers that may carry an
// objective use the three-argument launch_composite below: with a null record it IS composite.hip's launch_composite (kernels.h and
// composite.hip are untouched), so a context that never asks for an objective runs composite_kernel as before.
//
// Per ray, with pre_k the pre-clip colour, img_k = clip(pre_k, 0, 1), d_k = img_k - target_k, w_i the weights, acc = sum w_i,
// delta_i = t_{i+1} - t_i (last: 1e-10) and m_i = (t_i - t_0) + delta_i / 2:
//   photometric   mean over R*3 of rho(d);  gi_k = gate * grad_scale * (rho'(d_k) / 2)          (mse: rho'(d) / 2 = d, the plain kernel's)
//       mse d^2 | mae |d|, sign(0) = 0 | huber(D) d^2/2 inside |d| <= D, D (|d| - D/2) outside | log_cosh |d| + log1p(e^(-2|d|)) - ln 2
//   distortion    D = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i    (mip-NeRF 360), in O(S) for non-decreasing t:
//       with W_k = sum_{j<k} w_j, M_k = sum_{j<k} w_j m_j and the suffix sums W'_k = acc - W_k - w_k, M'_k = sum w m - M_k - w_k m_k
//       D = 2 sum_k w_k (m_k W_k - M_k) + 1/3 sum_k w_k^2 delta_k,   dD/dw_k = 2 (m_k W_k - M_k + M'_k - m_k W'_k) + 2/3 w_k delta_k
//   entropy       a = clamp(acc, 1e-4, 1 - 1e-4), H = -a ln a - (1 - a) ln(1 - a), dH/dw_k = ln((1 - a) / a) inside the clamp (inclusive), else 0
// The regularisers' gradient reg_scale (lambda_d dD/dw_k + lambda_e dH/dw_k) is added to dw BEHIND the clip gate (the gate belongs
// to the colour's clip; the weights are not clipped) and ahead of the suffix scan.  t carries no gradient.
#pragma once
#include <hip/hip_runtime.h>

namespace knerf {

struct CompositeArgs;

struct CompositeExt {
    int loss_kind;          // KNERF_LOSS_*
    float huber_delta;
    float lambda_d;         // distortion weight of THIS pass (0 where the record's `nets` leaves the pass's net out)
    float lambda_e;         // opacity-entropy weight of this pass
    float reg_scale;        // inv_chunks / R: scale of the regularisers' gradient, of their loss terms and of terms[2], terms[3]
    float* terms;           // [4] accumulators: photometric, squared error (both * loss_scale), distortion, entropy (both * reg_scale)
    float* terms_partial;   // deterministic mode: [4][ceil(R/4)] per-workgroup terms instead of four atomics per workgroup; or null
};

// ext == nullptr: composite.hip's launch_composite(a, stream), the plain kernel; else composite_ext_kernel<C> (training passes only)
hipError_t launch_composite(const CompositeArgs& a, const CompositeExt* ext, hipStream_t stream);
// deterministic mode: terms[k] += partial[k][0] + partial[k][1] + ... (fixed order), k = 0..3
hipError_t launch_terms_reduce(const float* partial, int n, float* terms, hipStream_t stream);

}  // namespace knerf
