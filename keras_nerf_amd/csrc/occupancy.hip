// occupancy.hip -- empty-space skipping for the render passes (gfx950).  Extension, no reference counterpart (occupancy grids as in
// Instant-NGP and Plenoxels: one bit per cell of a box).
//
// A render pass of n = R*S samples behind a grid (knerf_set_occupancy) runs:
//   occ_mark_kernel   p = o + d t (mlp_fwd.hip's two roundings), the cell lookup of include/knerf.h, raw = (0,0,0,0) at the dead
//                     samples, one 64-bit ballot per 64 samples, live samples per workgroup, stats
//   occ_scan_kernel   one workgroup: exclusive prefix of the per-workgroup counts, the list's length
//   occ_emit_kernel   the live sample indices in ASCENDING order (ballots + prefix): the list is reproducible
// then the fused MLP on the list only (query.hip query_list_kernel).  The general-shape path runs its MLP over every sample and uses the
// mark kernel alone to zero the dead ones.  The grid (128^3: 256 KB) stays in L2.
//
// Training behind a grid (option "occupancy_train") runs the same mark / scan / emit, then csrc/train_list.hip.
//
// occ_build_kernel (knerf_occupancy_from_grid, not on the hot path): a cell is occupied if one of its 8 lattice corners has
// sigma > threshold, then dilated by `dilation` cells (Chebyshev): i.e. any lattice point of the cell's box grown by `dilation` on every
// side, clipped to the lattice.  One thread per cell, one ballot per 64 cells = two words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/knerf.h"
#include "occupancy.h"

namespace knerf {

__global__ __launch_bounds__(kOccBlock) void occ_mark_kernel(OccArgs a) {
    __shared__ int s_cnt[kOccBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long base = (long long)blockIdx.x * kOccSpan;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kOccPer; ++k) {
        const long long g = base + k * kOccBlock + tid;
        bool live = false;
        if (g < a.n) {
            const long long ray = g / a.S;
            const float t = a.t[g];
            const float px = __fadd_rn(a.o[ray * 3 + 0], __fmul_rn(a.d[ray * 3 + 0], t));
            const float py = __fadd_rn(a.o[ray * 3 + 1], __fmul_rn(a.d[ray * 3 + 1], t));
            const float pz = __fadd_rn(a.o[ray * 3 + 2], __fmul_rn(a.d[ray * 3 + 2], t));
            live = occ_lookup(a.grid, px, py, pz);
            if (!live) reinterpret_cast<float4*>(a.raw)[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const unsigned long long m = __ballot(live);
        const long long w0 = base + k * kOccBlock + wv * 64;          // this wave's 64 samples: word w0 / 64 of the ballots
        if (a.masks && lane == 0 && w0 < a.n) a.masks[w0 >> 6] = m;
        cnt += __popcll(m);
    }
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < kOccBlock / 64; ++w) tot += s_cnt[w];
        if (a.blk_cnt) a.blk_cnt[blockIdx.x] = tot;
        if (a.stats) {
            if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats), (unsigned long long)tot);
            if (blockIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats + 1), (unsigned long long)a.n);
        }
    }
}

// one workgroup of 1024: exclusive prefix of the per-workgroup counts (wave scans, then the 16 wave totals), the total into *count
__global__ __launch_bounds__(1024) void occ_scan_kernel(const int* cnt, int nblk, int* off, int* count) {
    __shared__ int s_wave[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int base = 0, par = 0;
    for (int c0 = 0; c0 < nblk; c0 += 1024) {
        const int i = c0 + tid;
        const int v = i < nblk ? cnt[i] : 0;
        int x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_wave[par][wv] = x;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int s = s_wave[par][w]; woff += w < wv ? s : 0; tot += s; }
        if (i < nblk) off[i] = base + woff + x - v;
        base += tot;
        par ^= 1;                                            // the other buffer next time: one barrier per chunk is enough
    }
    if (tid == 0) *count = base;
}

// the live samples of workgroup span b in ascending order at list[off[b] ..]: the span's 32 ballots are in sample order
__global__ __launch_bounds__(kOccBlock) void occ_emit_kernel(OccArgs a) {
    constexpr int kWords = kOccSpan / 64;
    __shared__ int s_pre[kWords];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long base = (long long)blockIdx.x * kOccSpan;
    if (tid < kWords) s_pre[tid] = base + 64 * tid < a.n ? __popcll(a.masks[(base >> 6) + tid]) : 0;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < kWords; ++w) { const int c = s_pre[w]; s_pre[w] = s; s += c; }
    }
    __syncthreads();
    const int b0 = a.blk_off[blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < kOccPer; ++k) {
        const long long g = base + k * kOccBlock + tid;
        if (g >= a.n) break;
        const int w = k * (kOccBlock / 64) + wv;
        const unsigned long long m = a.masks[(base >> 6) + w];
        if ((m >> lane) & 1ull) a.list[b0 + s_pre[w] + __popcll(m & below)] = (int)g;
    }
}

hipError_t launch_occupancy_mark(const OccArgs& a, hipStream_t stream) {
    const long long nb = occ_blocks(a.n);
    hipLaunchKernelGGL(occ_mark_kernel, dim3((unsigned)nb), dim3(kOccBlock), 0, stream, a);
    if (!a.masks) return hipGetLastError();
    hipLaunchKernelGGL(occ_scan_kernel, dim3(1), dim3(1024), 0, stream, a.blk_cnt, (int)nb, a.blk_off, a.count);
    hipLaunchKernelGGL(occ_emit_kernel, dim3((unsigned)nb), dim3(kOccBlock), 0, stream, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void occ_build_kernel(const float* sigma, int rx, int ry, int rz, float threshold, int dil, unsigned* bits) {
    const int cx = rx - 1, cy = ry - 1, cz = rz - 1;
    const long long ncell = (long long)cx * cy * cz;
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool occ = false;
    if (b < ncell) {
        const long long yz = (long long)cy * cz;
        const int i = (int)(b / yz), j = (int)((b - i * yz) / cz), k = (int)(b - i * yz - (long long)j * cz);
        // lattice points [max(0, i - dil), min(c, i + 1 + dil)] per axis: the corners of every cell within distance dil
        const int x0 = i - dil > 0 ? i - dil : 0, x1 = i + 1 + dil < cx ? i + 1 + dil : cx;
        const int y0 = j - dil > 0 ? j - dil : 0, y1 = j + 1 + dil < cy ? j + 1 + dil : cy;
        const int z0 = k - dil > 0 ? k - dil : 0, z1 = k + 1 + dil < cz ? k + 1 + dil : cz;
        for (int x = x0; x <= x1 && !occ; ++x)
            for (int y = y0; y <= y1 && !occ; ++y) {
                const float* row = sigma + ((long long)x * ry + y) * rz;
                for (int z = z0; z <= z1; ++z)
                    if (row[z] > threshold) { occ = true; break; }
            }
    }
    const unsigned long long m = __ballot(occ);               // b of lane 0 is a multiple of 64: lanes 0-31 / 32-63 are two words
    if ((lane == 0 || lane == 32) && b < ncell) bits[b >> 5] = (unsigned)(lane == 0 ? m : m >> 32);
}

hipError_t launch_occupancy_scan(const int* cnt, int nblk, int* off, int* count, hipStream_t stream) {
    hipLaunchKernelGGL(occ_scan_kernel, dim3(1), dim3(1024), 0, stream, cnt, nblk, off, count);
    return hipGetLastError();
}

hipError_t launch_occupancy_build(const float* sigma, int rx, int ry, int rz, float threshold, int dilation, unsigned* bits, hipStream_t stream) {
    const long long ncell = (long long)(rx - 1) * (ry - 1) * (rz - 1);
    hipLaunchKernelGGL(occ_build_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, stream, sigma, rx, ry, rz, threshold, dilation, bits);
    return hipGetLastError();
}

}  // namespace knerf

extern "C" int knerf_occupancy_from_grid(void* stream, const float* sigma, int rx, int ry, int rz, float threshold, int dilation, uint32_t* bits) {
    if (!sigma || !bits) return KNERF_ERR_INVALID;
    if (rx < 2 || ry < 2 || rz < 2 || rx > 1025 || ry > 1025 || rz > 1025) return KNERF_ERR_INVALID;     // 1..1024 cells per axis
    if (dilation < 0 || dilation > 8) return KNERF_ERR_INVALID;
    if (knerf::launch_occupancy_build(sigma, rx, ry, rz, threshold, dilation, reinterpret_cast<unsigned*>(bits), (hipStream_t)stream) != hipSuccess)
        return KNERF_ERR_HIP;
    return KNERF_OK;
}

namespace knerf {

// Instant-NGP's density EMA, on the device: state = max(decay * state, sigma) (OccupancyGridUpdater keeps one state per net)
__global__ __launch_bounds__(256) void occ_decay_max_kernel(float* state, const float* sigma, unsigned long long n, float decay) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    state[i] = fmaxf(__fmul_rn(decay, state[i]), sigma[i]);
}

}  // namespace knerf

extern "C" int knerf_occupancy_decay_max(void* stream, float* state, const float* sigma, uint64_t n, float decay) {
    if (!state || !sigma || n == 0 || n > (1ull << 40)) return KNERF_ERR_INVALID;
    if (!(decay >= 0.f && decay <= 1.f)) return KNERF_ERR_INVALID;
    hipLaunchKernelGGL(knerf::occ_decay_max_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, state, sigma,
                       (unsigned long long)n, decay);
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
