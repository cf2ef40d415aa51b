// termination.hip -- early ray termination for the render passes (gfx950).  Extension, no reference counterpart (as in Instant-NGP
// and most volume renderers: nothing behind a point where the transmittance T has dropped below a small eps can move the pixel by
// more than eps).
//
// A render pass with option "termination_threshold" eps > 0 works in segments of L samples (option "termination_segment"); on the fused
// path one round per segment k, with no host synchronisation between rounds:
//   term_mark_kernel  fold segment k - 1's raw into T[ray] (one fp32 product per sample, in ascending sample order, the x factor of
//                     composite.hip), cut the ray if T < eps, look up the occupancy grid (occupancy.h occ_lookup), raw = (0,0,0,0) at
//                     the dead samples of segment k, one 64-bit ballot per 64 samples, live samples per workgroup, stats
//   occ_scan_kernel   (occupancy.hip, launch_occupancy_scan) exclusive prefix of the per-workgroup counts, the list's length
//   term_emit_kernel  the live global sample indices (ray * S + i) of segment k in ASCENDING order
// then the fused MLP on that list (query.hip query_list_kernel, sized for R * L_k samples; the length is read on the device).
// A workgroup holds whole rays' segments: rays_per_block(L) rays, at most kTermSpan samples, so the fold and the cut of a ray stay
// inside one workgroup and T needs no atomics.
//
// term_walk_kernel is the general-shape path: behind its dense forward, one thread per ray walks the samples with the same products
// and the same cut rule and zeroes the terminated ones (the same outputs without the speed-up).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "termination.h"

namespace knerf {

// x_i = 1 - alpha_i + 1e-10 with alpha_i = 1 - exp(-sigma_i delta_i): the arithmetic of composite.hip, operation for operation
__device__ __forceinline__ float term_x(float sigma, float dl) {
    const float ex = expf(-__fmul_rn(sigma, dl));
    return __fadd_rn(__fsub_rn(1.f, __fsub_rn(1.f, ex)), 1e-10f);
}
// delta_i = t_{i+1} - t_i, the last one 1e-10 (composite.hip)
__device__ __forceinline__ float term_delta(const float* t, long long g, int i, int S) { return i + 1 < S ? __fsub_rn(t[g + 1], t[g]) : 1e-10f; }

__device__ __forceinline__ bool term_occupied(const TermArgs& a, long long ray, long long g) {
    if (!a.has_grid) return true;
    const float t = a.t[g];
    const float px = __fadd_rn(a.o[ray * 3 + 0], __fmul_rn(a.d[ray * 3 + 0], t));
    const float py = __fadd_rn(a.o[ray * 3 + 1], __fmul_rn(a.d[ray * 3 + 1], t));
    const float pz = __fadd_rn(a.o[ray * 3 + 2], __fmul_rn(a.d[ray * 3 + 2], t));
    return occ_lookup(a.grid, px, py, pz);
}

__global__ __launch_bounds__(kTermBlock) void term_mark_kernel(TermArgs a) {
    __shared__ float s_x[kTermSpan];
    __shared__ unsigned char s_alive[kTermSpan];
    __shared__ int s_cnt[kTermBlock / 64], s_occ[kTermBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = a.L, S = a.S, k = a.k;
    const int rpb = L >= kTermSpan ? 1 : kTermSpan / L;
    const int r0 = blockIdx.x * rpb;
    const int nr = a.R - r0 < rpb ? a.R - r0 : rpb;
    if (k > 0) {
        // segment k - 1 has L samples (only the last segment can be shorter): its x factors, sample-parallel
        const int i0 = (k - 1) * L;
        for (int e = tid; e < nr * L; e += kTermBlock) {
            const int rr = e / L, i = i0 + e - rr * L;
            const long long g = (long long)(r0 + rr) * S + i;
            s_x[e] = term_x(a.raw[g * 4 + 3], term_delta(a.t, g, i, S));
        }
        __syncthreads();
    }
    for (int rr = tid; rr < nr; rr += kTermBlock) {
        float T = 1.f;
        if (k > 0) {
            T = a.T[r0 + rr];
            for (int j = 0; j < L; ++j) T = __fmul_rn(T, s_x[rr * L + j]);     // the documented order: one sample at a time
        }
        a.T[r0 + rr] = T;
        s_alive[rr] = !(T < a.eps);
    }
    __syncthreads();
    const int i0 = k * L, Lk = S - i0 < L ? S - i0 : L;
    const int span = nr * Lk, n_it = (rpb * Lk + kTermBlock - 1) / kTermBlock;     // n_it: the same in every workgroup
    int cnt = 0, occ = 0;
    for (int it = 0; it < n_it; ++it) {
        const int e = it * kTermBlock + tid;
        bool live = false, occd = false;
        if (e < span) {
            const int rr = e / Lk, i = i0 + e - rr * Lk;
            const long long ray = r0 + rr, g = ray * S + i;
            occd = term_occupied(a, ray, g);
            live = occd && s_alive[rr];
            if (!live) reinterpret_cast<float4*>(a.raw)[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const unsigned long long m = __ballot(live);
        if (lane == 0) a.masks[(long long)blockIdx.x * kTermWords + it * (kTermBlock / 64) + wv] = m;
        cnt += __popcll(m);
        occ += __popcll(__ballot(occd));
    }
    if (lane == 0) { s_cnt[wv] = cnt; s_occ[wv] = occ; }
    __syncthreads();
    if (tid == 0) {
        int tot = 0, tot_occ = 0;
#pragma unroll
        for (int w = 0; w < kTermBlock / 64; ++w) { tot += s_cnt[w]; tot_occ += s_occ[w]; }
        a.blk_cnt[blockIdx.x] = tot;
        const unsigned long long n = (unsigned long long)a.R * (unsigned long long)Lk;
        if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats), (unsigned long long)tot);
        if (blockIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats + 1), n);
        if (a.occ_stats) {
            if (tot_occ) atomicAdd(reinterpret_cast<unsigned long long*>(a.occ_stats), (unsigned long long)tot_occ);
            if (blockIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.occ_stats + 1), n);
        }
    }
}

// the live samples of workgroup b in ascending order at list[off[b] ..]: its ballots are in (ray, sample) order
__global__ __launch_bounds__(kTermBlock) void term_emit_kernel(TermArgs a) {
    __shared__ int s_pre[kTermWords];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = a.L, S = a.S;
    const int rpb = L >= kTermSpan ? 1 : kTermSpan / L;
    const int r0 = blockIdx.x * rpb;
    const int i0 = a.k * L, Lk = S - i0 < L ? S - i0 : L;
    const int n_it = (rpb * Lk + kTermBlock - 1) / kTermBlock, words = n_it * (kTermBlock / 64);
    const unsigned long long* masks = a.masks + (long long)blockIdx.x * kTermWords;
    if (tid < kTermWords) s_pre[tid] = tid < words ? __popcll(masks[tid]) : 0;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < kTermWords; ++w) { const int c = s_pre[w]; s_pre[w] = s; s += c; }
    }
    __syncthreads();
    const int b0 = a.blk_off[blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int it = 0; it < n_it; ++it) {
        const int w = it * (kTermBlock / 64) + wv;
        const unsigned long long m = masks[w];
        if ((m >> lane) & 1ull) {                     // set bits lie below span: e < nr * Lk
            const int e = it * kTermBlock + tid;
            const int rr = e / Lk, i = i0 + e - rr * Lk;
            a.list[b0 + s_pre[w] + __popcll(m & below)] = (r0 + rr) * S + i;
        }
    }
}

hipError_t launch_termination_round(const TermArgs& a, hipStream_t stream) {
    const long long nb = term_blocks(a.R, a.L);
    hipLaunchKernelGGL(term_mark_kernel, dim3((unsigned)nb), dim3(kTermBlock), 0, stream, a);
    if (hipError_t e = launch_occupancy_scan(a.blk_cnt, (int)nb, a.blk_off, a.count, stream)) return e;
    hipLaunchKernelGGL(term_emit_kernel, dim3((unsigned)nb), dim3(kTermBlock), 0, stream, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(kTermBlock) void term_walk_kernel(TermArgs a) {
    __shared__ int s_cnt[kTermBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long ray = (long long)blockIdx.x * kTermBlock + tid;
    int n_eval = 0;
    if (ray < a.R) {
        const int S = a.S, L = a.L;
        const long long g0 = ray * S;
        float T = 1.f;
        int cut = S;
        for (int i = 0; i < S; ++i) {
            if (i > 0 && i % L == 0 && T < a.eps) { cut = i; break; }
            T = __fmul_rn(T, term_x(a.raw[(g0 + i) * 4 + 3], term_delta(a.t, g0 + i, i, S)));
        }
        for (int i = cut; i < S; ++i) reinterpret_cast<float4*>(a.raw)[g0 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.has_grid) {
            for (int i = 0; i < cut; ++i) n_eval += term_occupied(a, ray, g0 + i);
        } else {
            n_eval = cut;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_eval += __shfl_xor(n_eval, o, 64);
    if (lane == 0) s_cnt[wv] = n_eval;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < kTermBlock / 64; ++w) tot += s_cnt[w];
        if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats), (unsigned long long)tot);
        if (blockIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats + 1), (unsigned long long)a.R * (unsigned long long)a.S);
    }
}

hipError_t launch_termination_walk(const TermArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(term_walk_kernel, dim3((unsigned)((a.R + kTermBlock - 1) / kTermBlock)), dim3(kTermBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace knerf
