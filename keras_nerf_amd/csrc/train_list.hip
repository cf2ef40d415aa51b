// train_list.hip -- the training forward on a list of live samples (gfx950): empty-space skipping in training behind an occupancy
// grid (knerf_set_option "occupancy_train").  Extension, no reference counterpart (Instant-NGP-style trainers march only occupied cells).
//
// mlp_fwd_list_kernel<S, NET> is the SAVE instantiation of mlp_fwd_kernel (mlp_fwd.hip) with another prologue and exit:
//   prologue  compacted entry i reads sample g = list[i] of the pass; ray g / S, p = o + d * t[g] with the same two roundings
//   exit      the list's length is read on the device: a workgroup whose first entry lies at or past it leaves before it touches LDS or
//             the weight ring (blockIdx alone decides, so all 8 waves leave together); inside the last live workgroup the entries past
//             the length clamp to the last one, as `valid` does in mlp_fwd.hip
// The saved act / mask blocks go to compacted tile i / 32 in mlp_fwd.hip's layout, so mlp_bwd and wgrad read them unchanged; raw goes to
// raw[g] (compositing's input; csrc/occupancy.hip has zeroed the dead samples there), and the gather kernel behind compositing copies it
// to raw_c[i] (mlp_bwd's input) with dL/draw: a second store here would keep i live to the head, and that costs the widest extra shapes
// (e.g. 4,2,256,16,3) a 12-byte spill that the SAVE forward does not have.  The trunk /
// head body, encode() and the store schedule are copies: mlp_fwd.hip and chain.h stay exactly as the training kernels were built and
// checked (build.KERNEL_FILES, kernel_digest).  Compiled once per trunk shape like the other sliced kernels (build.py SLICED); slice 0
// also holds the dispatcher and the gather kernel that prepares the compacted backward.
#include "chain.h"
#include "kernels.h"
#include "layout.h"
#include "train_list.h"

namespace knerf {

// mlp_fwd.hip encode(), unchanged: sin / cos of 2^i * x with exact range reduction, straight into B-operand slots
template <int L, int NQ>
__device__ __forceinline__ void list_encode(float x, float y, float z, int h, bf16x8 (&out)[NQ]) {
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

// mlp_fwd.hip make_fwd_stores(), unchanged: the SAVE variant's store schedule (the kernel below issues exactly those stores)
template <class S>
constexpr StoreSched<S::kFwdStages> list_fwd_stores() {
    StoreSched<S::kFwdStages> t{};
    for (int st = 0; st < S::kFwdStages; ++st)
        t.st[st] = StoreStage{S::fwd_b0(st), S::fwd_nks(st), S::fwd_not(st), (st == S::NL || (st == 0 && !S::kSaveH0)) ? 0 : 2,
                              st == S::NL ? 0 : (st == S::NL - 1 ? 1 + S::kTrunkXQ + S::kDirQ : 1), 0};
    t.initial = S::kEncQ;
    return t;
}
template <class S> struct ListFwdWait { static constexpr WaitTable<S::kFwdBlocks> tab = make_wait_table<S::kFwdStages, S::kFwdBlocks>(list_fwd_stores<S>()); };

// NET only names the instantiation (0 = coarse pass, 1 = fine pass) for profiler summaries; S = the trunk shape (layout.h)
template <class S, int NET>
__global__ __launch_bounds__(kThreads, 2) void mlp_fwd_list_kernel(TrainListArgs la) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FwdArgs& a = la.f;
    float* bias_lds = reinterpret_cast<float*>(smem + kRingBytes);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int col = lane & 31, h = lane >> 5;

    // the list's length is known on the device only: a workgroup with nothing to do leaves before it touches LDS or the ring.  The test
    // depends on blockIdx alone, so all 8 waves (which share the ring's barriers) leave together.
    const long long n = *la.count;
    if ((long long)blockIdx.x * kWaves * kTile >= n) return;

    for (int i = tid; i < S::kFwdBiasTiles * 32; i += kThreads) bias_lds[i] = a.bias[i];

    const long long tile = (long long)blockIdx.x * kWaves + wave;       // compacted tile
    long long i = tile * kTile + col;
    const bool valid = i < n;
    if (!valid) i = n - 1;
    const long long g = la.list[i];                                     // sample of the pass
    const long long ray = g / a.S;
    const float t = a.t[g];
    const float ox = a.o[ray * 3 + 0], oy = a.o[ray * 3 + 1], oz = a.o[ray * 3 + 2];
    const float dx = a.d[ray * 3 + 0], dy = a.d[ray * 3 + 1], dz = a.d[ray * 3 + 2];
    // p = o + d * t  (two roundings, as mlp_fwd.hip)
    const float px = __fadd_rn(ox, __fmul_rn(dx, t)), py = __fadd_rn(oy, __fmul_rn(dy, t)), pz = __fadd_rn(oz, __fmul_rn(dz, t));
    __syncthreads();

    Ring ring{a.stream, smem, tid, wave};
    ring.prologue_issue();
    asm volatile("" ::: "memory");            // every store below stays behind the prologue's LDS-DMA (StoreSched counts on it)

    constexpr int QX = S::kEncQ, QD = S::kDirQ;
    bf16x8 enc[QX];
    list_encode<S::LX, QX>(px, py, pz, h, enc);

    char* act = a.act + act_tile_off<S>((size_t)KNERF_STORE_TILE(tile));
    char* maskp = a.mask + mask_tile_off<S>((size_t)KNERF_STORE_TILE(tile));
#pragma unroll
    for (int q = 0; q < QX; ++q) store_block(act, S::kActEnc + q, lane, enc[q]);

    ring.prologue_wait();
    Prefetch pf;
    pf.start<S::kFwdBlocks>(ring, lane);
    ListFwdWait<S> waits;

    constexpr int K = S::kKs, T = S::kOt;
    bf16x8 x[K], y[K];
    auto relu_epi = [&](bf16x8 (&out)[K], int layer, unsigned (&mbits)[4]) {
        return [&, layer](int ot, f32x16 acc) {
            pack_acc(acc, out[2 * ot], out[2 * ot + 1]);
            out[2 * ot] = relu_packed(out[2 * ot]);
            out[2 * ot + 1] = relu_packed(out[2 * ot + 1]);
            if (layer > 0 || S::kSaveH0) {
                store_block(act, S::act_h(layer) + 2 * ot, lane, out[2 * ot]);
                store_block(act, S::act_h(layer) + 2 * ot + 1, lane, out[2 * ot + 1]);
            }
            const unsigned m = relu_mask_bits(out[2 * ot], out[2 * ot + 1]);
            if (ot & 1) mbits[ot >> 1] |= m << 8; else mbits[ot >> 1] = m;
            if (ot == T - 1) store16_wt(maskp, (unsigned)(layer * kSavedBlockStride + mask_lane_off(lane)), u32x4{mbits[0], mbits[1], mbits[2], mbits[3]});
        };
    };
    unsigned mb[4] = {0u, 0u, 0u, 0u};
    auto bias_init = [&](int base) { return [&, base](int ot) { return bias_acc(bias_lds, base + ot, h); }; };

    dense_stage<0, QX, T, S::kFwdBlocks>(ring, pf, lane, grp, waits, bias_init(0), [&](int ks) { return enc[ks]; }, relu_epi(x, 0, mb));
    static_for<S::NL - 1>([&](auto l_) {
        constexpr int l = decltype(l_)::value + 1;
        auto run = [&](bf16x8 (&in)[K], bf16x8 (&out)[K]) {
            if constexpr (S::concat_in(l)) {
                bf16x8 encc[QX];
                list_encode<S::LX, QX>(px, py, pz, h, encc);
                dense_stage<S::fwd_b0(l), K + QX, T, S::kFwdBlocks>(ring, pf, lane, grp, waits, bias_init(T * l),
                                                                   [&](int ks) { return ks < K ? in[ks < K ? ks : 0] : encc[ks >= K ? ks - K : 0]; },
                                                                   relu_epi(out, l, mb));
            } else {
                dense_stage<S::fwd_b0(l), K, T, S::kFwdBlocks>(ring, pf, lane, grp, waits, bias_init(T * l), [&](int ks) { return in[ks]; },
                                                               relu_epi(out, l, mb));
            }
        };
        if constexpr (l % 2) run(x, y); else run(y, x);
    });
    constexpr int QH = S::kTrunkXQ;
    bf16x8 ench[QH > 0 ? QH : 1];
    if constexpr (QH > 0) {
        list_encode<S::LX, QX>(px, py, pz, h, ench);
#pragma unroll
        for (int q = 0; q < QH; ++q) store_block(act, S::kActHeadEnc + q, lane, ench[q]);
    }
    bf16x8 dirc[QD];
    list_encode<S::LD, QD>(dx, dy, dz, h, dirc);
#pragma unroll
    for (int q = 0; q < QD; ++q) store_block(act, S::kActDir + q, lane, dirc[q]);
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
                                        reinterpret_cast<f32x4*>(a.raw)[g] = r;
                                    }
                                });
    };
    if constexpr ((S::NL - 1) % 2) head(y); else head(x);
    ring_finish<S::kFwdBlocks>(ring, grp);
}

template <class S>
hipError_t launch_mlp_fwd_list_t(const TrainListArgs& a, hipStream_t stream) {
    const long long tiles = (a.f.n_samples + kTile - 1) / kTile;        // sized for every sample of the pass; the count decides on the device
    const int grid = (int)((tiles + kWaves - 1) / kWaves);
    const size_t lds = kRingBytes + S::kFwdBiasTiles * 32 * sizeof(float);
    static AttrOnce once;
    hipError_t ae = once([&]() -> hipError_t {
        const void* fns[2] = {reinterpret_cast<const void*>(mlp_fwd_list_kernel<S, 0>), reinterpret_cast<const void*>(mlp_fwd_list_kernel<S, 1>)};
        for (const void* f : fns) {
            hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    });
    if (ae != hipSuccess) return ae;
    if (a.f.net == 0) hipLaunchKernelGGL((mlp_fwd_list_kernel<S, 0>), dim3(grid), dim3(kThreads), lds, stream, a);
    else hipLaunchKernelGGL((mlp_fwd_list_kernel<S, 1>), dim3(grid), dim3(kThreads), lds, stream, a);
    return hipGetLastError();
}

#define KNERF_X(I, ...) KNERF_PICK(I, template, extern template) hipError_t launch_mlp_fwd_list_t<KNERF_SHAPE_T(__VA_ARGS__)>(const TrainListArgs&, hipStream_t);
KNERF_FUSED_SHAPES(KNERF_X)
#undef KNERF_X

#if KNERF_HAS_DISPATCH
hipError_t launch_mlp_fwd_list(const TrainListArgs& a, hipStream_t stream) {
    switch (a.f.shape) {
#define KNERF_X(I, ...) case I: return launch_mlp_fwd_list_t<KNERF_SHAPE_T(__VA_ARGS__)>(a, stream);
        KNERF_FUSED_SHAPES(KNERF_X)
#undef KNERF_X
        default: return hipErrorInvalidValue;
    }
}

// one thread per compacted entry of the pass's tiles (n_tiles * 32 threads, whole workgroups of 256: a tile is half a wave).  A sample
// is dead for the backward exactly as composite.hip decides it: dL/drgb == 0 and (dL/dsigma == 0 or sigma == 0).
__global__ __launch_bounds__(256) void occ_train_gather_kernel(const int* list, const int* count, const f32x4* raw, const f32x4* draw, f32x4* draw_c, f32x4* raw_c,
                                                                int* flags, long long n, long long n_tiles, int skip_dead) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long long L = *count;
    const long long Lpad = (L + kTile - 1) / kTile * kTile;
    bool live = false;
    if (i < L) {
        const int g = list[i];
        const f32x4 r = raw[g], v = draw[g];
        raw_c[i] = r;
        draw_c[i] = v;
        const bool dead = v[0] == 0.f && v[1] == 0.f && v[2] == 0.f && (v[3] == 0.f || r[3] == 0.f);
        live = !skip_dead || !dead;
    } else if (i < Lpad && i < n) {
        draw_c[i] = f32x4{0.f, 0.f, 0.f, 0.f};                        // the last tile's padding: finite and inert in mlp_bwd
        raw_c[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const unsigned long long m = __ballot(live);
    if ((lane == 0 || lane == 32) && i < n_tiles * kTile) {
        const long long tile = i / kTile;
        // a tile below ceil(L / 32) with no live entry is dead only when skipping applies; beyond it nothing is evaluated
        const bool any = (lane == 0 ? (unsigned)m : (unsigned)(m >> 32)) != 0u;
        flags[tile] = tile * kTile < L ? (skip_dead ? (int)any : 1) : 0;
    }
}

hipError_t launch_occupancy_train_gather(const int* list, const int* count, const float* raw, const float* draw, float* draw_c, float* raw_c, int* flags,
                                         long long n, long long n_tiles, int skip_dead, hipStream_t stream) {
    const long long threads = n_tiles * kTile;
    hipLaunchKernelGGL(occ_train_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, list, count,
                       reinterpret_cast<const f32x4*>(raw), reinterpret_cast<const f32x4*>(draw), reinterpret_cast<f32x4*>(draw_c), reinterpret_cast<f32x4*>(raw_c), flags, n, n_tiles,
                       skip_dead);
    return hipGetLastError();
}
#endif

}  // namespace knerf
