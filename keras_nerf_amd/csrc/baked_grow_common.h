// baked_grow_common.h -- the per-point arithmetic of growing a baked field, one text for dense and brick storage: baked_grow.hip
// (knerf_baked_resample, knerf_baked_train_tv) and baked_bricks_grow.hip (the same on bricks) differ in how a lattice point's record or
// row is found and in nothing else, so that both give the same bits.  A kernel finds its point and its neighbours; everything that
// rounds is here.
#pragma once
#include "baked_common.h"

namespace knerf {
namespace baked_grow {
using namespace baked;

// ---- resampling

// a (1 - f) + b f, every operation rounded on its own: f = 0 gives a and f = 1 gives b exactly
__device__ __forceinline__ float lerp(float a, float b, float f) { return __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, f)), __fmul_rn(b, f)); }

// where the new index i of an axis with rn points lies among the r old points: the old cell and the position inside it
__device__ __forceinline__ void place(int i, int r, int rn, int& cell, float& f) {
    const double u = (double)i * (double)(r - 1) / (double)(rn - 1);
    const int fl = (int)floor(u);
    cell = fl < r - 2 ? fl : r - 2;
    f = (float)(u - (double)cell);
}

// trilinear along z, then y, then x; c[4 dx + 2 dy + dz] is the value at corner (cx + dx, cy + dy, cz + dz) of the old cell
__device__ __forceinline__ float trilerp(const float (&c)[8], float fx, float fy, float fz) {
    const float l00 = lerp(c[0], c[1], fz), l01 = lerp(c[2], c[3], fz), l10 = lerp(c[4], c[5], fz), l11 = lerp(c[6], c[7], fz);
    return lerp(lerp(l00, l01, fy), lerp(l10, l11, fy), fx);
}

// a new sigma as it is stored
__device__ __forceinline__ float keep_sigma(float sigma, float threshold) { return sigma > threshold ? sigma : 0.f; }

__device__ __forceinline__ unsigned chunk_word(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// the new sigma from the first word of the 8 old records' chunk 0
__device__ __forceinline__ float resample_sigma(const unsigned (&first)[8], float fx, float fy, float fz, float threshold) {
    float c[8];
#pragma unroll
    for (int cn = 0; cn < 8; ++cn) c[cn] = __uint_as_float(first[cn]);
    return keep_sigma(trilerp(c, fx, fy, fz), threshold);
}

// the 16-byte chunk qc of a new record from the same chunk of the 8 old records (corner order as trilerp): fp32 sigma in front of chunk 0,
// coefficients fp16 -> fp32 -> fp16 (nearest even), zeros past the 3 K coefficients
__device__ __forceinline__ uint4 resample_chunk(const uint4 (&old)[8], int qc, int K, float fx, float fy, float fz, float threshold) {
    unsigned h[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        float c[8];
#pragma unroll
        for (int cn = 0; cn < 8; ++cn) c[cn] = half_bits_to_float(chunk_word(old[cn], s >> 1) >> ((s & 1) * 16));
        const int e = 8 * qc - 2 + s;
        h[s] = (e >= 0 && e < 3 * K) ? float_to_half_bits(trilerp(c, fx, fy, fz)) : 0u;
    }
    unsigned first[8];
#pragma unroll
    for (int cn = 0; cn < 8; ++cn) first[cn] = old[cn].x;
    uint4 out;
    out.x = qc == 0 ? __float_as_uint(resample_sigma(first, fx, fy, fz, threshold)) : (h[0] | (h[1] << 16));
    out.y = h[2] | (h[3] << 16);
    out.z = h[4] | (h[5] << 16);
    out.w = h[6] | (h[7] << 16);
    return out;
}

// ---- total variation over rows [.][W] of master values

// tv at a point with value v whose successors along x, y, z have the rows s[0..2] (-1: no difference along that axis); the
// differences come back in d
template <int W>
__device__ __forceinline__ float tv_term(const float* master, float eps, int q, float v, const long long (&s)[3], float (&d)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = s[c] >= 0 ? master[s[c] * W + q] - v : 0.f;
    return sqrtf(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + eps);
}

// column q of the row `row`: its tv term comes back and, where the weight w is not 0, the whole of g is formed in registers and added
// to grad with one fp32 add.  row_at(dx, dy, dz): the row of the point at that offset from this one, -1 where it lies outside the
// lattice or takes no part; it is asked for the 12 other points the gradient needs.
template <int W, class RowAt>
__device__ __forceinline__ float tv_column(const float* master, float* grad, float eps, float w, long long row, int q, RowAt&& row_at) {
    const long long at = row * W + q;
    const float v0 = master[at];
    float d[3];
    const long long s0[3] = {row_at(1, 0, 0), row_at(0, 1, 0), row_at(0, 0, 1)};
    const float tv0 = tv_term<W>(master, eps, q, v0, s0, d);
    if (w != 0.f) {
        float acc = 0.f - ((d[0] + d[1]) + d[2]) / tv0;      // (0 - x, not -x: where every difference is 0, g is +0)
        // the predecessors: along axis c the successor of p - e_c is p itself
        const long long sx = row_at(-1, 0, 0);
        if (sx >= 0) {
            const long long s[3] = {row, row_at(-1, 1, 0), row_at(-1, 0, 1)};
            const float tv = tv_term<W>(master, eps, q, master[sx * W + q], s, d);
            acc = acc + d[0] / tv;
        }
        const long long sy = row_at(0, -1, 0);
        if (sy >= 0) {
            const long long s[3] = {row_at(1, -1, 0), row, row_at(0, -1, 1)};
            const float tv = tv_term<W>(master, eps, q, master[sy * W + q], s, d);
            acc = acc + d[1] / tv;
        }
        const long long sz = row_at(0, 0, -1);
        if (sz >= 0) {
            const long long s[3] = {row_at(1, 0, -1), row_at(0, 1, -1), row};
            const float tv = tv_term<W>(master, eps, q, master[sz * W + q], s, d);
            acc = acc + d[2] / tv;
        }
        grad[at] = grad[at] + w * acc;                       // the one add
    }
    return tv0;
}

// tv_out of the rows of a block: every lane brings its term (0 where it has none), the row's first lane sums the others in column order
// in double and stores both.  Every lane of the block comes here.
template <int W>
__device__ __forceinline__ void tv_store(float (&terms)[kBlock], int t, bool first_of_valid_row, float tv0, float* tv_out, long long row) {
    terms[t] = tv0;
    __syncthreads();
    if (first_of_valid_row) {
        double sum = 0.0;
        for (int j = 1; j < W; ++j) sum += (double)terms[t + j];
        tv_out[row * 2] = tv0;
        tv_out[row * 2 + 1] = (float)sum;
    }
}

// the arguments both TV entry points check alike
inline bool check_tv(float weight_sigma, float weight_sh, float epsilon) {
    if (!(epsilon > 0.f) || !std::isfinite(epsilon)) return false;
    return weight_sigma >= 0.f && std::isfinite(weight_sigma) && weight_sh >= 0.f && std::isfinite(weight_sh);
}

}  // namespace baked_grow
}  // namespace knerf
