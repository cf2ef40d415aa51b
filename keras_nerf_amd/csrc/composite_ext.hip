// composite_ext.hip -- composite.hip's training kernel with the extended objective of composite_ext.h (gfx950): a photometric term
// other than the squared error (mae, huber, log-cosh) and the distortion / opacity-entropy regularisers of the ray's weights.
//
// The same kernel as composite_kernel<C> -- one wavefront per ray, a lane-local run of C samples, the transmittance as a wave-level
// exclusive product scan, the mirrored suffix scan of the backward, the same early exit of the waves beyond R through the barriers,
// the same dead-sample rule, tile flags and list append -- with three additions:
//   * rho(d) and rho'(d) / 2 in place of d^2 and d (for mse they ARE d^2 and d: the same operations, the same bits);
//   * two forward wave scans (exclusive sums of w and of w m, built like the transmittance scan: lane totals, six __shfl_up steps)
//     and the totals through wave_sum, from which every sample gets dD/dw_k in O(1);
//   * the regularisers' gradient added to dw ahead of pr = dw w -- only when a weight is non-zero, so that an objective without a
//     regulariser forms exactly the plain kernel's dw (x + 0 would turn a -0 into +0).
// Four terms per ray (photometric, squared error, distortion, entropy) leave with one atomic per workgroup each, or as
// per-workgroup partials in deterministic mode (terms_reduce_kernel adds them in a fixed order).
#include <hip/hip_runtime.h>

#include "../../include/knerf.h"
#include "composite_ext.h"
#include "kernels.h"

namespace knerf {

typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int C>
__global__ __launch_bounds__(256) void composite_ext_kernel(CompositeArgs a, CompositeExt e) {
    __shared__ float s_loss[4], s_terms[4][4];
    __shared__ int s_cnt[4], s_base[2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ray = blockIdx.x * 4 + wv;
    if (lane == 0) { s_loss[wv] = 0.f; s_cnt[wv] = 0; s_terms[0][wv] = 0.f; s_terms[1][wv] = 0.f; s_terms[2][wv] = 0.f; s_terms[3][wv] = 0.f; }
    if (ray >= a.R) {         // whole wave leaves together; it still joins the block's reductions and list append
        __syncthreads(); if (a.tile_list) { __syncthreads(); __syncthreads(); }
        return;
    }
    const int S = a.S;
    const float eps = 1e-10f;
    const f32x4* raw = reinterpret_cast<const f32x4*>(a.raw) + (size_t)ray * S;
    const float* t = a.t + (size_t)ray * S;
    const float t0 = t[0];    // m is taken relative to the ray's first sample: D is shift-invariant, and most of the fp32 cancellation goes

    float r[C], g[C], b[C], sg[C], tt[C], dl[C], ex[C], x[C], T[C], w[C];
    float run = 1.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int i = lane * C + c;
        const bool ok = i < S;
        f32x4 v = ok ? raw[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        r[c] = v[0]; g[c] = v[1]; b[c] = v[2]; sg[c] = v[3];
        tt[c] = ok ? t[i] : 0.f;
        const float tn = (i + 1 < S) ? t[i + 1] : 0.f;
        dl[c] = (i + 1 < S) ? __fsub_rn(tn, tt[c]) : eps;
        ex[c] = expf(-__fmul_rn(sg[c], dl[c]));
        w[c] = ok ? __fsub_rn(1.f, ex[c]) : 0.f;      // alpha, until the scan below
        x[c] = ok ? __fadd_rn(__fsub_rn(1.f, w[c]), eps) : 1.f;
        T[c] = run;               // lane-local exclusive product
        run *= x[c];
    }
    float inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        float u = __shfl_up(inc, o, 64);
        if (lane >= o) inc *= u;
    }
    float excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = 1.f;
    float sr = 0.f, sgc = 0.f, sb = 0.f, sd = 0.f, sw = 0.f, lm = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        T[c] *= excl;
        w[c] = w[c] * T[c];
        sr += w[c] * r[c]; sgc += w[c] * g[c]; sb += w[c] * b[c];
        sd += w[c] * tt[c]; sw += w[c];
        lm += w[c] * ((tt[c] - t0) + 0.5f * dl[c]);
    }
    const float lw = sw;      // this lane's total weight, before the butterfly
    sr = wave_sum(sr); sgc = wave_sum(sgc); sb = wave_sum(sb); sd = wave_sum(sd); sw = wave_sum(sw);
    float pre[3] = {sr, sgc, sb};
    if (a.white & 1) { const float bg = 1.f - sw; pre[0] += bg; pre[1] += bg; pre[2] += bg; }
    float img[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) img[k] = (a.white & 2) ? pre[k] : fminf(fmaxf(pre[k], 0.f), 1.f);
    if (lane < 3) a.image[(size_t)ray * 3 + lane] = lane == 0 ? img[0] : (lane == 1 ? img[1] : img[2]);
    if (a.depth && lane == 0) a.depth[ray] = sd;
    if (a.weights) {
#pragma unroll
        for (int c = 0; c < C; ++c) { const int i = lane * C + c; if (i < S) a.weights[(size_t)ray * S + i] = w[c]; }
    }

    // ---- photometric term: rho(d) summed, gi = gate * grad_scale * rho'(d) / 2
    float gi[3], l2 = 0.f, lp = 0.f;
    const float hd = e.huber_delta;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float df = img[k] - a.target[(size_t)ray * 3 + k];
        const float ad = fabsf(df);
        l2 += df * df;
        float rho, h;
        switch (e.loss_kind) {
            case KNERF_LOSS_MAE: rho = ad; h = df > 0.f ? 0.5f : (df < 0.f ? -0.5f : 0.f); break;
            case KNERF_LOSS_HUBER: rho = ad <= hd ? 0.5f * (df * df) : hd * (ad - 0.5f * hd); h = 0.5f * fminf(fmaxf(df, -hd), hd); break;
            case KNERF_LOSS_LOG_COSH: rho = (ad + log1pf(expf(-2.f * ad))) - 0.693147180559945f; h = 0.5f * tanhf(df); break;
            default: rho = df * df; h = df; break;
        }
        lp += rho;
        gi[k] = (pre[k] >= 0.f && pre[k] <= 1.f) ? a.grad_scale * h : 0.f;
    }

    // ---- distortion: exclusive wave scans of the lanes' sum w and sum w m, totals through the butterfly
    float incw = lw, incm = lm;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float uw = __shfl_up(incw, o, 64), um = __shfl_up(incm, o, 64);
        if (lane >= o) { incw += uw; incm += um; }
    }
    float Wr = __shfl_up(incw, 1, 64), Mr = __shfl_up(incm, 1, 64);     // running exclusive prefix sums W_k, M_k
    if (lane == 0) { Wr = 0.f; Mr = 0.f; }
    const float Mtot = wave_sum(lm);
    // ---- opacity entropy of acc = sum w
    const float lo = 1e-4f, hi = 1.f - 1e-4f;
    const float ac = fminf(fmaxf(sw, lo), hi);
    const float H = -ac * logf(ac) - (1.f - ac) * logf(1.f - ac);
    const float dH = (sw >= lo && sw <= hi) ? logf((1.f - ac) / ac) : 0.f;
    const bool has_reg = e.lambda_d != 0.f || e.lambda_e != 0.f;        // uniform

    const float gsum = (a.white & 1) ? (gi[0] + gi[1] + gi[2]) : 0.f;
    float dw[C];
    float dpart = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        dw[c] = gi[0] * r[c] + gi[1] * g[c] + gi[2] * b[c] - gsum;
        const float m = (tt[c] - t0) + 0.5f * dl[c];
        const float wm = w[c] * m;
        const float before = m * Wr - Mr;                               // sum_{j<k} w_j (m_k - m_j)
        const float Ws = (sw - Wr) - w[c], Ms = (Mtot - Mr) - wm;       // suffix sums W'_k, M'_k
        const float gD = 2.f * ((before + Ms) - m * Ws) + 0.666666666666667f * (w[c] * dl[c]);
        dpart += 2.f * (w[c] * before) + 0.333333333333333f * ((w[c] * w[c]) * dl[c]);
        if (has_reg) dw[c] += e.reg_scale * (e.lambda_d * gD + e.lambda_e * dH);      // not through the clip gate
        Wr += w[c]; Mr += wm;
    }
    const float tD = wave_sum(dpart) * e.reg_scale, tH = H * e.reg_scale;
    float lray = lp * a.loss_scale;
    if (has_reg) lray += e.lambda_d * tD + e.lambda_e * tH;
    if (lane == 0) { s_loss[wv] = lray; s_terms[0][wv] = lp * a.loss_scale; s_terms[1][wv] = l2 * a.loss_scale; s_terms[2][wv] = tD; s_terms[3][wv] = tH; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float l4 = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
        if (a.loss_partial) a.loss_partial[blockIdx.x] = l4;
        else atomicAdd(a.loss, l4);
    }
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        const float t4 = (s_terms[k][0] + s_terms[k][1]) + (s_terms[k][2] + s_terms[k][3]);
        if (e.terms_partial) e.terms_partial[(size_t)k * gridDim.x + blockIdx.x] = t4;
        else atomicAdd(e.terms + k, t4);
    }

    float pr[C], Ql[C];
    float suffix = 0.f;            // lane-local exclusive suffix sums of dw*w, built right to left
#pragma unroll
    for (int c = C - 1; c >= 0; --c) {
        pr[c] = dw[c] * w[c];
        Ql[c] = suffix;
        suffix += pr[c];
    }
    float incs = suffix;           // wave reverse inclusive scan of lane totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        float u = __shfl_down(incs, o, 64);
        if (lane + o < 64) incs += u;
    }
    float excls = __shfl_down(incs, 1, 64);
    if (lane == 63) excls = 0.f;
    f32x4* draw = reinterpret_cast<f32x4*>(a.draw) + (size_t)ray * S;
    unsigned live = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int i = lane * C + c;
        if (i < S) {
            const float Q = Ql[c] + excls;
            const float dalpha = dw[c] * T[c] - Q / x[c];
            const float dsig = dalpha * dl[c] * ex[c];
            const f32x4 v = f32x4{w[c] * gi[0], w[c] * gi[1], w[c] * gi[2], dsig};
            draw[i] = v;
            // composite.hip's dead-sample rule: it reads draw and sigma only, so it holds for any objective
            const bool dead = v[0] == 0.f && v[1] == 0.f && v[2] == 0.f && (v[3] == 0.f || sg[c] == 0.f);
            if (!dead) live |= 1u << (i >> 5);
        }
    }
    if (a.tile_flags || a.tile_list) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) live |= __shfl_xor(live, o, 64);
    }
    const int nt = S >> 5;
    if (a.tile_flags && lane < nt) a.tile_flags[(size_t)ray * nt + lane] = (live >> lane) & 1u;
    if (a.tile_list) {
        if (lane == 0) s_cnt[wv] = __popc(live);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int tot = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
            s_base[0] = tot ? atomicAdd(a.tile_count, tot) : 0;
            s_base[1] = (tot && a.tile_list2) ? atomicAdd(a.tile_count2, tot) : 0;
        }
        __syncthreads();
        int off = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) off += k < wv ? s_cnt[k] : 0;
        if (lane < nt && ((live >> lane) & 1u)) {
            const int rr = off + __popc(live & ((1u << lane) - 1u)), id = ray * nt + lane;
            a.tile_list[s_base[0] + rr] = id;
            if (a.tile_list2) a.tile_list2[s_base[1] + rr] = id + a.tile_off2;
        }
    }
}

// deterministic mode: wave k adds the workgroups' k-th terms in a fixed order
__global__ __launch_bounds__(256) void terms_reduce_kernel(const float* partial, int n, float* terms) {
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += partial[(size_t)k * n + i];
    s = wave_sum(s);
    if (lane == 0) terms[k] += s;
}

}  // namespace

hipError_t launch_terms_reduce(const float* partial, int n, float* terms, hipStream_t stream) {
    hipLaunchKernelGGL(terms_reduce_kernel, dim3(1), dim3(256), 0, stream, partial, n, terms);
    return hipGetLastError();
}

hipError_t launch_composite(const CompositeArgs& a, const CompositeExt* ext, hipStream_t stream) {
    if (!ext) return launch_composite(a, stream);                            // the plain objective: composite.hip, untouched
    const CompositeExt& e = *ext;
    if (!a.draw || !a.target || !e.terms) return hipErrorInvalidValue;      // the training half only
    const int grid = (a.R + 3) / 4;
    const int C = (a.S + 63) / 64;
    switch (C) {
        case 1: hipLaunchKernelGGL(composite_ext_kernel<1>, dim3(grid), dim3(256), 0, stream, a, e); break;
        case 2: hipLaunchKernelGGL(composite_ext_kernel<2>, dim3(grid), dim3(256), 0, stream, a, e); break;
        case 3: hipLaunchKernelGGL(composite_ext_kernel<3>, dim3(grid), dim3(256), 0, stream, a, e); break;
        case 4: hipLaunchKernelGGL(composite_ext_kernel<4>, dim3(grid), dim3(256), 0, stream, a, e); break;
        case 5: case 6: case 7: case 8: hipLaunchKernelGGL(composite_ext_kernel<8>, dim3(grid), dim3(256), 0, stream, a, e); break;
        case 9: case 10: case 11: case 12: hipLaunchKernelGGL(composite_ext_kernel<12>, dim3(grid), dim3(256), 0, stream, a, e); break;
        case 13: case 14: case 15: case 16: hipLaunchKernelGGL(composite_ext_kernel<16>, dim3(grid), dim3(256), 0, stream, a, e); break;
        default: return hipErrorInvalidValue;   // more than 1024 samples per ray
    }
    return hipGetLastError();
}

}  // namespace knerf
