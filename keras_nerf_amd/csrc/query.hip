// query.hip -- the trained field at arbitrary points: fused positional encoding + trunk + collapsed head in inference mode (gfx950).
// Extension, no reference counterpart (the original NeRF release evaluates its fine network on a dense grid to extract a mesh).
//
// query_kernel<S> is the inference instantiation of mlp_fwd_kernel (mlp_fwd.hip) with another prologue and epilogue: the same
// weight stream, ring, dense stages and head, so a point gives the bits the render path gives the same sample.  The trunk / head
// body is a copy, not a shared function: mlp_fwd.hip and chain.h stay exactly as the training kernels were built and checked.
//   prologue  points: xyz [n,3]; grid: point g = (i,j,k) of a [R0,R1,R2] grid (C order, z fastest) at
//             __fadd_rn(lo, __fmul_rn((float)idx, step)) per axis (csrc/mesh.hip places vertices on the same lattice).
//             Direction: none (zero vector), one shared [3], or per point [n,3].
//             List mode (query_list_kernel): sample list[g] of a render pass, p and direction exactly as mlp_fwd.hip computes them
//             (the occupancy grid's live samples, csrc/occupancy.hip); the list's length is read on the device.
//   epilogue  raw [n,4] (rgb after sigmoid, sigma after relu), and / or sigma [n], rgb [n,3].
// Compiled once per trunk shape like the other sliced kernels (build.py SLICED); slice 0 also holds the dispatcher and the
// general-shape route's gather / scatter kernels.
#include "chain.h"
#include "kernels.h"
#include "layout.h"
#include "query.h"

namespace knerf {

// mlp_fwd.hip encode(), unchanged: sin / cos of 2^i * x with exact range reduction, straight into B-operand slots
template <int L, int NQ>
__device__ __forceinline__ void query_encode(float x, float y, float z, int h, bf16x8 (&out)[NQ]) {
    const float C1 = 0.15915494f;             // fl(1/(2 pi))
    const float C2 = 6.4206383e-09f;          // 1/(2 pi) - C1
    float v[3] = {x, y, z};
    float rh[3], rl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        rh[c] = v[c] * C1;
        rl[c] = __builtin_fmaf(v[c], C1, -rh[c]) + v[c] * C2;
    }
    static_assert(2 + 3 * L <= NQ * 8, "encode: NQ k-steps hold 8 NQ features per lane half");
    const float phase = h ? 0.25f : 0.0f;
    float e[NQ * 8];
#pragma unroll
    for (int m = 0; m < NQ * 8; ++m) e[m] = 0.f;
    e[0] = h ? z : x;
    e[1] = h ? 0.f : y;
#pragma unroll
    for (int i = 0; i < L; ++i) {
        const float s = (float)(1 << i);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float a = rh[c] * s;
            float f = a - __builtin_floorf(a);
            float arg = f + (rl[c] * s + phase);
            e[2 + 3 * i + c] = __builtin_amdgcn_sinf(arg);
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) out[q][j] = (__bf16)e[8 * q + j];
}

constexpr StoreSched<1> kQueryNoStores = {{{0, 1, 0, 0, 0, 0}}, 0};
template <class S> struct QueryWait { static constexpr WaitTable<S::kFwdBlocks> tab = make_wait_table<1, S::kFwdBlocks>(kQueryNoStores); };

// point gi of the query: its coordinates and direction
__device__ __forceinline__ void query_point(const QueryArgs& a, long long gi, float (&p)[3], float (&d)[3]) {
    if (a.grid) {
        const long long yz = (long long)a.gr[1] * a.gr[2];
        const long long i = gi / yz, r = gi - i * yz, j = r / a.gr[2], k = r - j * a.gr[2];
        p[0] = __fadd_rn(a.lo[0], __fmul_rn((float)i, a.step[0]));
        p[1] = __fadd_rn(a.lo[1], __fmul_rn((float)j, a.step[1]));
        p[2] = __fadd_rn(a.lo[2], __fmul_rn((float)k, a.step[2]));
    } else {
        p[0] = a.xyz[gi * 3 + 0]; p[1] = a.xyz[gi * 3 + 1]; p[2] = a.xyz[gi * 3 + 2];
    }
    if (a.dir) {
        const long long o = gi * a.dir_stride;
        d[0] = a.dir[o + 0]; d[1] = a.dir[o + 1]; d[2] = a.dir[o + 2];
    } else {
        d[0] = d[1] = d[2] = 0.f;
    }
}

__device__ __forceinline__ void query_store(const QueryArgs& a, long long gi, const f32x4& r) {
    if (a.raw) reinterpret_cast<f32x4*>(a.raw)[gi] = r;
    if (a.sigma) a.sigma[gi] = r[3];
    if (a.rgb) { a.rgb[gi * 3 + 0] = r[0]; a.rgb[gi * 3 + 1] = r[1]; a.rgb[gi * 3 + 2] = r[2]; }
}

// LIST = false: points / grid prologue (query_kernel); true: the render pass's live samples (query_list_kernel, below)
template <class S, bool LIST>
__device__ __forceinline__ void query_body(const QueryArgs& a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* bias_lds = reinterpret_cast<float*>(smem + kRingBytes);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int col = lane & 31, h = lane >> 5;

    long long n = a.n;
    if constexpr (LIST) {
        // the list's length is known on the device only: a workgroup with nothing to do leaves before it touches LDS or the ring.
        // The test depends on blockIdx alone, so all 8 waves (which share the ring's barriers) leave together.
        n = *a.count;
        if ((long long)blockIdx.x * kWaves * kTile >= n) return;
    }

    for (int i = tid; i < S::kFwdBiasTiles * 32; i += kThreads) bias_lds[i] = a.bias[i];

    const long long tile = (long long)blockIdx.x * kWaves + wave;
    long long g = tile * kTile + col;
    const bool valid = g < n;
    if (!valid) g = n - 1;
    long long gi;
    float p[3], dv[3];
    if constexpr (LIST) {
        gi = a.list[g];
        const long long ray = gi / a.S;
        const float t = a.t[gi];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dv[c] = a.d[ray * 3 + c];
            p[c] = __fadd_rn(a.o[ray * 3 + c], __fmul_rn(dv[c], t));     // mlp_fwd.hip: two roundings
        }
    } else {
        gi = a.offset + g;
        query_point(a, gi, p, dv);
    }
    const float px = p[0], py = p[1], pz = p[2], dx = dv[0], dy = dv[1], dz = dv[2];
    __syncthreads();

    Ring ring{a.stream, smem, tid, wave};
    ring.prologue_issue();
    asm volatile("" ::: "memory");

    constexpr int QX = S::kEncQ, QD = S::kDirQ;
    bf16x8 enc[QX];
    query_encode<S::LX, QX>(px, py, pz, h, enc);

    ring.prologue_wait();
    Prefetch pf;
    pf.start<S::kFwdBlocks>(ring, lane);
    QueryWait<S> waits;

    constexpr int K = S::kKs, T = S::kOt;
    bf16x8 x[K], y[K];
    auto relu_epi = [&](bf16x8 (&out)[K]) {
        return [&](int ot, f32x16 acc) {
            pack_acc(acc, out[2 * ot], out[2 * ot + 1]);
            out[2 * ot] = relu_packed(out[2 * ot]);
            out[2 * ot + 1] = relu_packed(out[2 * ot + 1]);
        };
    };
    auto bias_init = [&](int base) { return [&, base](int ot) { return bias_acc(bias_lds, base + ot, h); }; };

    dense_stage<0, QX, T, S::kFwdBlocks>(ring, pf, lane, grp, waits, bias_init(0), [&](int ks) { return enc[ks]; }, relu_epi(x));
    static_for<S::NL - 1>([&](auto l_) {
        constexpr int l = decltype(l_)::value + 1;
        auto run = [&](bf16x8 (&in)[K], bf16x8 (&out)[K]) {
            if constexpr (S::concat_in(l)) {
                bf16x8 encc[QX];
                query_encode<S::LX, QX>(px, py, pz, h, encc);
                dense_stage<S::fwd_b0(l), K + QX, T, S::kFwdBlocks>(ring, pf, lane, grp, waits, bias_init(T * l),
                                                                   [&](int ks) { return ks < K ? in[ks < K ? ks : 0] : encc[ks >= K ? ks - K : 0]; },
                                                                   relu_epi(out));
            } else {
                dense_stage<S::fwd_b0(l), K, T, S::kFwdBlocks>(ring, pf, lane, grp, waits, bias_init(T * l), [&](int ks) { return in[ks]; },
                                                               relu_epi(out));
            }
        };
        if constexpr (l % 2) run(x, y); else run(y, x);
    });
    constexpr int QH = S::kTrunkXQ;
    bf16x8 ench[QH > 0 ? QH : 1];
    if constexpr (QH > 0) query_encode<S::LX, QX>(px, py, pz, h, ench);
    bf16x8 dirc[QD];
    query_encode<S::LD, QD>(dx, dy, dz, h, dirc);
    auto head = [&](bf16x8 (&in)[K]) {
        dense_stage<S::fwd_b0(S::NL), K + QH + QD, 1, S::kFwdBlocks>(ring, pf, lane, grp, waits, bias_init(T * S::NL),
                                [&](int ks) { return ks < K ? in[ks < K ? ks : 0] : (ks < K + QH ? ench[(ks >= K && ks < K + QH) ? ks - K : 0] : dirc[ks >= K + QH ? ks - K - QH : 0]); },
                                [&](int, f32x16 acc) {
                                    if (valid && h == 0) {
                                        f32x4 r;
                                        r[0] = 1.f / (1.f + expf(-acc[0]));
                                        r[1] = 1.f / (1.f + expf(-acc[1]));
                                        r[2] = 1.f / (1.f + expf(-acc[2]));
                                        r[3] = acc[3] > 0.f ? acc[3] : 0.f;
                                        query_store(a, gi, r);
                                    }
                                });
    };
    if constexpr ((S::NL - 1) % 2) head(y); else head(x);
    ring_finish<S::kFwdBlocks>(ring, grp);
}

template <class S>
__global__ __launch_bounds__(kThreads, 2) void query_kernel(QueryArgs a) { query_body<S, false>(a); }

// the third prologue: raw of the live samples of a render pass (csrc/occupancy.hip builds the list)
template <class S>
__global__ __launch_bounds__(kThreads, 2) void query_list_kernel(QueryArgs a) { query_body<S, true>(a); }

template <class S>
hipError_t launch_query_t(const QueryArgs& a, hipStream_t stream) {
    const long long tiles = (a.n + kTile - 1) / kTile;
    const int grid = (int)((tiles + kWaves - 1) / kWaves);
    const size_t lds = kRingBytes + S::kFwdBiasTiles * 32 * sizeof(float);
    static AttrOnce once;
    hipError_t ae = once([&]() -> hipError_t {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(query_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    if (ae != hipSuccess) return ae;
    hipLaunchKernelGGL((query_kernel<S>), dim3(grid), dim3(kThreads), lds, stream, a);
    return hipGetLastError();
}

template <class S>
hipError_t launch_query_list_t(const QueryArgs& a, hipStream_t stream) {
    const long long tiles = (a.n + kTile - 1) / kTile;           // sized for every sample of the pass; the count decides on the device
    const int grid = (int)((tiles + kWaves - 1) / kWaves);
    const size_t lds = kRingBytes + S::kFwdBiasTiles * 32 * sizeof(float);
    static AttrOnce once;
    hipError_t ae = once([&]() -> hipError_t {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(query_list_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    if (ae != hipSuccess) return ae;
    hipLaunchKernelGGL((query_list_kernel<S>), dim3(grid), dim3(kThreads), lds, stream, a);
    return hipGetLastError();
}

#define KNERF_X(I, ...) KNERF_PICK(I, template, extern template) hipError_t launch_query_t<KNERF_SHAPE_T(__VA_ARGS__)>(const QueryArgs&, hipStream_t); \
    KNERF_PICK(I, template, extern template) hipError_t launch_query_list_t<KNERF_SHAPE_T(__VA_ARGS__)>(const QueryArgs&, hipStream_t);
KNERF_FUSED_SHAPES(KNERF_X)
#undef KNERF_X

#if KNERF_HAS_DISPATCH
hipError_t launch_query(const QueryArgs& a, hipStream_t stream) {
    switch (a.shape) {
#define KNERF_X(I, ...) case I: return launch_query_t<KNERF_SHAPE_T(__VA_ARGS__)>(a, stream);
        KNERF_FUSED_SHAPES(KNERF_X)
#undef KNERF_X
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_query_list(const QueryArgs& a, hipStream_t stream) {
    switch (a.shape) {
#define KNERF_X(I, ...) case I: return launch_query_list_t<KNERF_SHAPE_T(__VA_ARGS__)>(a, stream);
        KNERF_FUSED_SHAPES(KNERF_X)
#undef KNERF_X
        default: return hipErrorInvalidValue;
    }
}

__global__ void query_gather_kernel(QueryArgs a, long long n, float* xyz, float* dir) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    float p[3], d[3];
    query_point(a, a.offset + g, p, d);
#pragma unroll
    for (int c = 0; c < 3; ++c) { xyz[3 * g + c] = p[c]; dir[3 * g + c] = d[c]; }
}

__global__ void query_scatter_kernel(QueryArgs a, long long n, const float* raw) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    query_store(a, a.offset + g, reinterpret_cast<const f32x4*>(raw)[g]);
}

hipError_t launch_query_gather(const QueryArgs& a, long long n, float* xyz, float* dir, hipStream_t stream) {
    hipLaunchKernelGGL(query_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, n, xyz, dir);
    return hipGetLastError();
}

hipError_t launch_query_scatter(const QueryArgs& a, long long n, const float* raw, hipStream_t stream) {
    hipLaunchKernelGGL(query_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, n, raw);
    return hipGetLastError();
}
#endif

}  // namespace knerf
