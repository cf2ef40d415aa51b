// baked_grow.hip -- what turns the fine-tuner of baked_train.hip into a grid trainer (gfx950), context-free: a total-variation
// regulariser over the slots of an optimiser and the resampling of a field onto another lattice (coarse to fine).  Extension: the
// reference has nothing of the kind (Plenoxels and its kin regularise and refine their grids in this way).  include/knerf.h holds
// the contract; tests/baked_grow_reference.py is its NumPy restatement.  The record's sizes and codec and the lattice check are those
// of baked_common.h.
//
//   baked_tv_kernel <W>       one lane per (slot, column) of the rows [n_slots][W], W = 1 + 3 K = 4 / 13 / 28 / 49.  A block of 256
//                             lanes holds floor(256 / W) WHOLE rows (256 / 247 / 252 / 245 lanes at work), so that consecutive lanes
//                             read consecutive floats, rows straddle waves but never blocks, and the per-slot sums of tv_out are a
//                             block-local matter (LDS, summed in a fixed order by the row's first lane: plain stores, no atomics).
//                             A lane reads its column in the 13 rows the gradient needs (the point, its three successors, its three
//                             predecessors and their two other successors each), reached through slot_of, forms the whole of g in
//                             registers and adds it to grad with one fp32 add: the launch is a gather and deterministic.
//   baked_resample_kernel     one lane per (new point, 16-byte chunk), as baked_train_apply_kernel: the chunk of the 8 surrounding old
//                             records, trilinear z, y, x with lerp(a, b, f) = a (1 - f) + b f in separate roundings (f = 0 returns a,
//                             f = 1 returns b, exactly), the position of the new point on each axis computed in double.
#include "baked_common.h"

namespace knerf {
namespace baked_grow {
using namespace baked;

struct TvArgs {
    const int* slot_of;
    const int* point_of;
    const float* master;
    float* grad;
    float* tv_out;
    long long n_slots, n_points;
    int R[3];
    float w_sigma, w_sh, eps;
};

// the slot of lattice point (x, y, z), -1 outside the lattice, without a slot, or with a slot number the rows do not have
__device__ __forceinline__ long long slot_at(const TvArgs& a, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= a.R[0] || y >= a.R[1] || z >= a.R[2]) return -1;
    const long long s = a.slot_of[((long long)x * a.R[1] + y) * a.R[2] + z];
    return s < a.n_slots ? s : -1;
}

// tv at a point with value v whose successors along x, y, z have the slots s[0..2] (-1: no difference along that axis); the
// differences come back in d
template <int W>
__device__ __forceinline__ float tv_term(const TvArgs& a, int q, float v, const long long (&s)[3], float (&d)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = s[c] >= 0 ? a.master[s[c] * W + q] - v : 0.f;
    return sqrtf(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + a.eps);
}

template <int W>
__global__ __launch_bounds__(kBlock) void baked_tv_kernel(TvArgs a) {
    constexpr int S = kBlock / W;                        // whole rows per block
    __shared__ float terms[kBlock];
    const int t = threadIdx.x;
    const int ls = t / W, q = t - ls * W;
    const long long slot = (long long)blockIdx.x * S + ls;
    const bool valid = ls < S && slot < a.n_slots;
    const float w = q == 0 ? a.w_sigma : a.w_sh;
    float tv0 = 0.f;
    if (valid && (w != 0.f || a.tv_out)) {
        const long long p = a.point_of[slot];
        if (p >= 0 && p < a.n_points) {
            const long long at = slot * W + q;
            const int z = (int)(p % a.R[2]);
            const long long xy = p / a.R[2];
            const int y = (int)(xy % a.R[1]), x = (int)(xy / a.R[1]);
            const float v0 = a.master[at];
            float d[3];
            const long long s0[3] = {slot_at(a, x + 1, y, z), slot_at(a, x, y + 1, z), slot_at(a, x, y, z + 1)};
            tv0 = tv_term<W>(a, q, v0, s0, d);
            if (w != 0.f) {
                float acc = 0.f - ((d[0] + d[1]) + d[2]) / tv0;      // (0 - x, not -x: where every difference is 0, g is +0)
                // the predecessors: along axis c the successor of p - e_c is p itself
                const long long sx = slot_at(a, x - 1, y, z);
                if (sx >= 0) {
                    const long long s[3] = {slot, slot_at(a, x - 1, y + 1, z), slot_at(a, x - 1, y, z + 1)};
                    const float tv = tv_term<W>(a, q, a.master[sx * W + q], s, d);
                    acc = acc + d[0] / tv;
                }
                const long long sy = slot_at(a, x, y - 1, z);
                if (sy >= 0) {
                    const long long s[3] = {slot_at(a, x + 1, y - 1, z), slot, slot_at(a, x, y - 1, z + 1)};
                    const float tv = tv_term<W>(a, q, a.master[sy * W + q], s, d);
                    acc = acc + d[1] / tv;
                }
                const long long sz = slot_at(a, x, y, z - 1);
                if (sz >= 0) {
                    const long long s[3] = {slot_at(a, x + 1, y, z - 1), slot_at(a, x, y + 1, z - 1), slot};
                    const float tv = tv_term<W>(a, q, a.master[sz * W + q], s, d);
                    acc = acc + d[2] / tv;
                }
                a.grad[at] = a.grad[at] + w * acc;       // the one add
            }
        }
    }
    if (a.tv_out) {                                      // the same for every lane of the launch
        terms[t] = tv0;
        __syncthreads();
        if (valid && q == 0) {
            double sum = 0.0;
            for (int j = 1; j < W; ++j) sum += (double)terms[t + j];
            a.tv_out[slot * 2] = tv0;
            a.tv_out[slot * 2 + 1] = (float)sum;
        }
    }
}

template <int W>
hipError_t launch_tv(const TvArgs& a, hipStream_t s) {
    constexpr int S = kBlock / W;
    const long long blocks = (a.n_slots + S - 1) / S;
    if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((baked_tv_kernel<W>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

struct ResampleArgs {
    const uint4* src;
    uint4* dst;
    int R[3], Rn[3];
    int K, nch;
    long long n_new;
    float threshold;
};

// a (1 - f) + b f, every operation rounded on its own: f = 0 gives a and f = 1 gives b exactly
__device__ __forceinline__ float lerp(float a, float b, float f) { return __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, f)), __fmul_rn(b, f)); }

// where the new index i of an axis with rn points lies among the r old points: the old cell and the position inside it
__device__ __forceinline__ void place(int i, int r, int rn, int& cell, float& f) {
    const double u = (double)i * (double)(r - 1) / (double)(rn - 1);
    const int fl = (int)floor(u);
    cell = fl < r - 2 ? fl : r - 2;
    f = (float)(u - (double)cell);
}

__global__ __launch_bounds__(kBlock) void baked_resample_kernel(ResampleArgs a) {
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= a.n_new * a.nch) return;
    const long long pn = idx / a.nch;
    const int qc = (int)(idx - pn * a.nch);
    const int k = (int)(pn % a.Rn[2]);
    const long long ij = pn / a.Rn[2];
    const int j = (int)(ij % a.Rn[1]), i = (int)(ij / a.Rn[1]);
    int cx, cy, cz;
    float fx, fy, fz;
    place(i, a.R[0], a.Rn[0], cx, fx);
    place(j, a.R[1], a.Rn[1], cy, fy);
    place(k, a.R[2], a.Rn[2], cz, fz);
    float plane[2][8], sig_plane[2];                     // per x corner: the chunk's 8 values (and sigma) after the z and y steps
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
        float line[2][8], sig_line[2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const long long pt = ((long long)(cx + dx) * a.R[1] + (cy + dy)) * a.R[2] + cz;
            const uint4 lo = a.src[pt * a.nch + qc], hi = a.src[(pt + 1) * a.nch + qc];
            const unsigned wl[4] = {lo.x, lo.y, lo.z, lo.w}, wh[4] = {hi.x, hi.y, hi.z, hi.w};
            sig_line[dy] = lerp(__uint_as_float(wl[0]), __uint_as_float(wh[0]), fz);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                line[dy][s] = lerp(half_bits_to_float(wl[s >> 1] >> ((s & 1) * 16)), half_bits_to_float(wh[s >> 1] >> ((s & 1) * 16)), fz);
            }
        }
        sig_plane[dx] = lerp(sig_line[0], sig_line[1], fy);
#pragma unroll
        for (int s = 0; s < 8; ++s) plane[dx][s] = lerp(line[0][s], line[1][s], fy);
    }
    unsigned h[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int e = 8 * qc - 2 + s;
        h[s] = (e >= 0 && e < 3 * a.K) ? float_to_half_bits(lerp(plane[0][s], plane[1][s], fx)) : 0u;
    }
    const float sig = lerp(sig_plane[0], sig_plane[1], fx);
    uint4 out;
    out.x = qc == 0 ? __float_as_uint(sig > a.threshold ? sig : 0.f) : (h[0] | (h[1] << 16));
    out.y = h[2] | (h[3] << 16);
    out.z = h[4] | (h[5] << 16);
    out.w = h[6] | (h[7] << 16);
    a.dst[idx] = out;
}

}  // namespace baked_grow
}  // namespace knerf

using namespace knerf;

extern "C" int knerf_baked_train_tv(void* stream, const knerf_baked_train* train, const int32_t* point_of, const float* master,
                                    float weight_sigma, float weight_sh, float epsilon, float* tv_out) {
    // the struct errors of knerf_baked_train_apply
    if (!train || !train->field.records || !train->field.bits || !train->slot_of || !train->grad || !point_of || !master)
        return KNERF_ERR_INVALID;
    unsigned long long points = 0;
    if (!baked::check_lattice(train->field.resolution, train->field.lo, train->field.hi, train->field.sh_degree, nullptr, points))
        return KNERF_ERR_INVALID;
    if (train->n_slots < 1 || train->n_slots > points) return KNERF_ERR_INVALID;
    if (!(epsilon > 0.f) || !std::isfinite(epsilon)) return KNERF_ERR_INVALID;
    if (!(weight_sigma >= 0.f) || !std::isfinite(weight_sigma) || !(weight_sh >= 0.f) || !std::isfinite(weight_sh)) return KNERF_ERR_INVALID;
    if (weight_sigma == 0.f && weight_sh == 0.f && !tv_out) return KNERF_OK;      // nothing to add, nothing to report
    baked_grow::TvArgs a{};
    a.slot_of = train->slot_of; a.point_of = point_of; a.master = master; a.grad = train->grad; a.tv_out = tv_out;
    a.n_slots = (long long)train->n_slots; a.n_points = (long long)points;
    for (int c = 0; c < 3; ++c) a.R[c] = train->field.resolution[c];
    a.w_sigma = weight_sigma; a.w_sh = weight_sh; a.eps = epsilon;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipErrorInvalidValue;
    switch (train->field.sh_degree) {
        case 0: e = baked_grow::launch_tv<4>(a, s); break;
        case 1: e = baked_grow::launch_tv<13>(a, s); break;
        case 2: e = baked_grow::launch_tv<28>(a, s); break;
        case 3: e = baked_grow::launch_tv<49>(a, s); break;
    }
    return e == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_resample(void* stream, const knerf_baked_field* src, const int32_t dst_resolution[3], float sigma_threshold,
                                    void* dst_records) {
    if (!src || !src->records || !dst_resolution || !dst_records) return KNERF_ERR_INVALID;
    unsigned long long points = 0, points_new = 0;
    const int deg = src->sh_degree;
    if (!baked::check_lattice(src->resolution, src->lo, src->hi, deg, nullptr, points)) return KNERF_ERR_INVALID;
    if (!baked::check_lattice(dst_resolution, src->lo, src->hi, deg, nullptr, points_new)) return KNERF_ERR_INVALID;     // (the same box)
    if (!(sigma_threshold >= 0.f) || !std::isfinite(sigma_threshold)) return KNERF_ERR_INVALID;
    const unsigned long long rb = (unsigned)baked::rec_bytes(deg);
    const uintptr_t s0 = (uintptr_t)src->records, d0 = (uintptr_t)dst_records;
    if (s0 < d0 + points_new * rb && d0 < s0 + points * rb) return KNERF_ERR_INVALID;      // the tables overlap
    baked_grow::ResampleArgs a{};
    a.src = static_cast<const uint4*>(src->records); a.dst = static_cast<uint4*>(dst_records);
    for (int c = 0; c < 3; ++c) { a.R[c] = src->resolution[c]; a.Rn[c] = dst_resolution[c]; }
    a.K = baked::n_coeff(deg); a.nch = (int)(rb / 16);
    a.n_new = (long long)points_new; a.threshold = sigma_threshold;
    const unsigned long long blocks = (points_new * (unsigned)a.nch + baked::kBlock - 1) / baked::kBlock;
    if (blocks >= (1ull << 31)) return KNERF_ERR_INVALID;
    hipLaunchKernelGGL(baked_grow::baked_resample_kernel, dim3((unsigned)blocks), dim3(baked::kBlock), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
