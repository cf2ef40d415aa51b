// baked_quant.hip -- the brick baked field with 8-bit SH coefficients: its codec and its renderer (gfx950), context-free.
// Extension: the reference has nothing of the kind (PlenOctrees and SNeRG ship their SH coefficients as 8-bit values with a scale).
// include/knerf.h holds the format (knerf_baked_qbricks); tests/baked_quant_reference.py restates it in NumPy.  What the file shares
// with the other baked*.hip files (sh_eval, the DPP sums, locate, the argument checks) is in baked_common.h.
//
// A quantised record is fp32 sigma + 3 K int8 [k][c], padded with zeros to 8 / 16 / 32 / 64 bytes (degree 0 / 1 / 2 / 3); coefficient
// e = 3 k + c is byte 4 + e.  One exponent per stored brick and SH band l = floor(sqrt(k)), byte l of the brick's exponent word:
// dec = q 2^e, exact in fp32 and exactly an fp16 number.
//
//   baked_quantize_bricks_kernel   <DEG>: one workgroup per stored brick.  Every lane takes the band maxima of its records as |fp16| BITS
//                          (they order like the magnitudes; a NaN counts as 0), the maxima are reduced by wave shuffles and across the
//                          waves through LDS -- a maximum does not depend on the order, so the result is the same on every launch; no
//                          atomics, no host read.  Every lane then forms the exponents, lane 0 writes the word, and the records are
//                          read again (from L2) and written quantised.
//   baked_dequantize_bricks_kernel <DEG>: one lane per record: sigma's bits, the coefficients as q 2^e in fp16 (exact), zero padding.
//   baked_render_qbricks_kernel    <DEG, G>: the march of baked_render_kernel (baked.hip) on brick storage, word for word -- sample
//                          positions, locate, corner order, the table lookup with its range guard and one-entry cache, batches of kBatch
//                          occupancy words, termination, stats, clamps, the fused multiply-adds -- with another fetch: the record is
//                          8 .. 64 bytes, the exponent word of a corner's brick is loaded by slot beside the record (and cached with the
//                          slot), and every corner's coefficients are decoded to fp32 BEFORE they enter fma(w, coeff, acc): the 8 corners
//                          may lie in 8 bricks with 8 different exponents.  G = 1 accumulates in ascending e = 3 k + c exactly as
//                          baked_render_kernel<DEG, 1, BrickRenderArgs> does, so it gives the bits of that kernel on the dequantised field
//                          (tests/test_gpu_baked_quant.py holds the two in step).  G = 2 (degree 2) / 4 (degree 3): every lane of a
//                          group takes one 16-byte chunk of the record and folds the power of two into the corner's weight (w 2^e is
//                          exact, so fma(q, w 2^e, acc) rounds the same exact product once); the channel sums go through the DPP
//                          pattern.
#include "baked_common.h"

namespace knerf {
namespace quant {
using namespace baked;

constexpr int kExpMin = -24, kExpMax = 9;           // 2^-24: the fp16 subnormal spacing; 127 x 2^9 = 65024 <= 65504

__host__ __device__ constexpr int qrec_bytes(int deg) { return deg == 0 ? 8 : (deg == 1 ? 16 : (deg == 2 ? 32 : 64)); }
// the SH band of coefficient slot e = 3 k + c: floor(sqrt(k))
__host__ __device__ constexpr int band_of(int e) { return (e >= 3) + (e >= 12) + (e >= 27); }
static_assert(qrec_bytes(0) >= 4 + 3 * n_coeff(0) && qrec_bytes(1) >= 4 + 3 * n_coeff(1) && qrec_bytes(2) >= 4 + 3 * n_coeff(2) &&
              qrec_bytes(3) >= 4 + 3 * n_coeff(3), "a quantised record holds sigma and 3 K bytes");

__device__ __forceinline__ float pow2(int e) { return __int_as_float((e + 127) << 23); }            // -126 <= e <= 127
// 2^e of the exponent byte at bit `shift` of a brick's exponent word; a byte outside [-24, 9] (a damaged table) is clamped into it, so
// that every decoded value stays finite
__device__ __forceinline__ float band_scale(unsigned word, int shift) {
    int e = (int)((word >> shift) << 24) >> 24;
    e = e < kExpMin ? kExpMin : (e > kExpMax ? kExpMax : e);
    return pow2(e);
}

// ---------------------------------------------------------------------------------------------------------------- the codec
template <int DEG>
__global__ __launch_bounds__(kBlock) void baked_quantize_bricks_kernel(const uint4* __restrict__ src, unsigned* __restrict__ dst,
                                                                       unsigned* __restrict__ exps, int places) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, QW = qrec_bytes(DEG) / 4;
    __shared__ unsigned smax[kBlock / 64][4];
    const long long first = (long long)blockIdx.x * places;
    unsigned m[DEG + 1];
#pragma unroll
    for (int l = 0; l <= DEG; ++l) m[l] = 0u;
    for (int p = threadIdx.x; p < places; p += blockDim.x) {
        const uint4* r = src + (first + p) * NCH;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const uint4 v = r[j];
            const unsigned wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int e = 8 * j - 2 + s;
                if (e >= 0 && e < 3 * K) {
                    unsigned h = (wd[s >> 1] >> ((s & 1) * 16)) & 0x7fffu;
                    h = h > 0x7c00u ? 0u : h;                                   // a NaN counts as 0
                    m[band_of(e)] = h > m[band_of(e)] ? h : m[band_of(e)];
                }
            }
        }
    }
    const int n_waves = (int)blockDim.x >> 6, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int l = 0; l <= DEG; ++l) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)m[l], off, 64);
            m[l] = o > m[l] ? o : m[l];
        }
        if ((threadIdx.x & 63) == 0) smax[wave][l] = m[l];
    }
    __syncthreads();
    int ex[DEG + 1];
    unsigned word = 0u;
#pragma unroll
    for (int l = 0; l <= DEG; ++l) {
        unsigned M = 0u;
        for (int w = 0; w < n_waves; ++w) M = smax[w][l] > M ? smax[w][l] : M;
        const float Mf = half_bits_to_float(M);                                 // +inf stays +inf: e = 9
        int e = kExpMin;
        while (e < kExpMax && 127.f * pow2(e) < Mf) ++e;                        // the smallest e with 127 x 2^e >= M (exact products)
        ex[l] = e;
        word |= ((unsigned)e & 0xffu) << (8 * l);
    }
    if (threadIdx.x == 0) exps[blockIdx.x] = word;
    for (int p = threadIdx.x; p < places; p += blockDim.x) {
        const uint4* r = src + (first + p) * NCH;
        unsigned out[QW];
#pragma unroll
        for (int i = 0; i < QW; ++i) out[i] = 0u;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const uint4 v = r[j];
            const unsigned wd[4] = {v.x, v.y, v.z, v.w};
            if (j == 0) out[0] = wd[0];                                         // sigma, bit for bit
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int e = 8 * j - 2 + s;
                if (e >= 0 && e < 3 * K) {
                    const float c = half_bits_to_float(wd[s >> 1] >> ((s & 1) * 16));
                    const float t = __builtin_rintf(__fmul_rn(c, pow2(-ex[band_of(e)])));           // exact product, nearest even
                    const int q = c != c ? 0 : (int)fminf(fmaxf(t, -127.f), 127.f);
                    out[(4 + e) >> 2] |= ((unsigned)q & 0xffu) << (8 * ((4 + e) & 3));
                }
            }
        }
        unsigned* d = dst + (first + p) * QW;
        if constexpr (QW == 2) {
            *reinterpret_cast<uint2*>(d) = make_uint2(out[0], out[1]);
        } else {
#pragma unroll
            for (int i = 0; i < QW; i += 4) *reinterpret_cast<uint4*>(d + i) = make_uint4(out[i], out[i + 1], out[i + 2], out[i + 3]);
        }
    }
}

template <int DEG>
__global__ __launch_bounds__(kBlock) void baked_dequantize_bricks_kernel(const unsigned* __restrict__ src, const unsigned* __restrict__ exps,
                                                                         uint4* __restrict__ dst, long long n_records, int log2_places) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, QW = qrec_bytes(DEG) / 4;
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= n_records) return;
    const unsigned ew = exps[idx >> log2_places];
    unsigned q[QW];
    if constexpr (QW == 2) {
        const uint2 v = *reinterpret_cast<const uint2*>(src + idx * QW);
        q[0] = v.x; q[1] = v.y;
    } else {
#pragma unroll
        for (int i = 0; i < QW; i += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + idx * QW + i);
            q[i] = v.x; q[i + 1] = v.y; q[i + 2] = v.z; q[i + 3] = v.w;
        }
    }
    float sc[DEG + 1];
#pragma unroll
    for (int l = 0; l <= DEG; ++l) sc[l] = band_scale(ew, 8 * l);
    unsigned out[NCH * 4];
#pragma unroll
    for (int i = 0; i < NCH * 4; ++i) out[i] = 0u;
    out[0] = q[0];
#pragma unroll
    for (int e = 0; e < 3 * K; ++e) {
        const int b = (int)((q[(4 + e) >> 2] >> (8 * ((4 + e) & 3))) << 24) >> 24;
        const _Float16 h = (_Float16)__fmul_rn((float)b, sc[band_of(e)]);       // exact: |q| <= 128, 2^-24 <= scale <= 2^9
        out[(2 + e) >> 1] |= (unsigned)__builtin_bit_cast(unsigned short, h) << (16 * ((2 + e) & 1));
    }
#pragma unroll
    for (int j = 0; j < NCH; ++j) dst[idx * NCH + j] = make_uint4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
}

// ---------------------------------------------------------------------------------------------------------------- the march
struct RenderArgs {
    const unsigned char* rec;
    const unsigned* exps;
    const int* brick_of;
    const unsigned* bits;
    int R[3];
    int L, By, Bz;                                  // log2 of the brick edge; the brick grid's y and z extents
    long long n_bricks;
    float lo[3], hi[3], scale[3];
    const float *o, *d, *near, *far;
    float near0, far0;
    long long n;
    float step, eps;
    int white, skip;
    float *image, *depth, *opacity;
    unsigned long long* stats;
};

// A lane of a group holds bytes 16 sub .. 16 sub + 15 of the record, coefficient slots e = 16 sub - 4 + s.  Its 16 bytes fall into three
// runs, [0, 7), [7, 15) and [15, 16), inside each of which every coefficient slot of every lane has ONE band (lane 0: bands 0, 1, 1;
// lane 1: 2, 2, 3; lanes 2 and 3: 3, 3, 3), so a lane needs three scales per corner, picked by constants of the lane.
__host__ __device__ constexpr int seg_of(int s) { return s < 7 ? 0 : (s < 15 ? 1 : 2); }
__host__ __device__ constexpr int seg_first(int g) { return g == 0 ? 4 : (g == 1 ? 7 : 15); }      // a byte of the run that is a slot in lane 0 too
constexpr bool segments_hold() {
    for (int sub = 0; sub < 4; ++sub)
        for (int s = 0; s < 16; ++s) {
            const int e = 16 * sub - 4 + s;
            if (e >= 0 && e < 48 && band_of(e) != band_of(16 * sub - 4 + seg_first(seg_of(s)))) return false;
        }
    return true;
}
static_assert(segments_hold(), "every run of a lane's 16 bytes lies in one SH band");

template <int DEG, int G>
__global__ __launch_bounds__(kBlock) void baked_render_qbricks_kernel(RenderArgs a) {
    constexpr int K = n_coeff(DEG), QB = qrec_bytes(DEG), NW = QB / 4 / G, NS = 4 * NW;     // words / byte slots of a record per lane
    static_assert(G == 1 || (G == 2 && DEG == 2) || (G == 4 && DEG == 3), "a group takes one 16-byte chunk per lane");
    static_assert(G == 1 || NW == 4, "a group takes one 16-byte chunk per lane");
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long ray = gid / G;
    const int sub = (int)(gid & (G - 1));
    unsigned long long fetched = 0, total = 0;
    if (ray < a.n) {
        const float ox = a.o[ray * 3 + 0], oy = a.o[ray * 3 + 1], oz = a.o[ray * 3 + 2];
        const float dx = a.d[ray * 3 + 0], dy = a.d[ray * 3 + 1], dz = a.d[ray * 3 + 2];
        const float near = a.near ? a.near[ray] : a.near0, far = a.far ? a.far[ray] : a.far0;
        const float nrm = __fsqrt_rn(dx * dx + dy * dy + dz * dz);
        const float ux = nrm > 0.f ? dx / nrm : 0.f, uy = nrm > 0.f ? dy / nrm : 0.f, uz = nrm > 0.f ? dz / nrm : 0.f;
        float Y[K];
        sh_eval<DEG>(ux, uy, uz, Y);
        // G > 1, constant along the ray: the basis value of each of this lane's 16 byte slots (0 for sigma's bytes and the padding: a
        // record's padding is never trusted, and every byte decodes to a finite number), the bit offsets of its three runs' exponent
        // bytes, and by how much its channels are rotated: slot s carries channel (s + 2 + sub) mod 3
        [[maybe_unused]] float yk[NS];
        [[maybe_unused]] int sh[3] = {0, 0, 0}, rot = 0;
        if constexpr (G > 1) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int e = NS * sub - 4 + s;
                const int k = e / 3;
                float v = 0.f;
#pragma unroll
                for (int kk = 0; kk < K; ++kk) v = (e >= 0 && k == kk) ? Y[kk] : v;
                yk[s] = v;
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const int e = NS * sub - 4 + seg_first(g);
                const int l = (e >= 3) + (e >= 12) + (e >= 27);
                sh[g] = 8 * (l < DEG ? l : DEG);                    // (a run of padding only: any band the degree has)
            }
            rot = sub % 3;
        }
        const double q = ((double)far - (double)near) / (double)a.step;
        const int S = q > 0.0 ? (q >= (double)kMaxSamples ? kMaxSamples : (int)ceil(q)) : 0;
        if (sub == 0) total = (unsigned long long)S;
        // slab intersection: only narrows the index range
        const float o3[3] = {ox, oy, oz}, d3[3] = {dx, dy, dz};
        float tmin = -INFINITY, tmax = INFINITY;
        bool miss = false;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (d3[c] == 0.f) {
                if (o3[c] < a.lo[c] || o3[c] > a.hi[c]) miss = true;
            } else {
                const float t1 = (a.lo[c] - o3[c]) / d3[c], t2 = (a.hi[c] - o3[c]) / d3[c];
                tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
            }
        }
        int i = 0, i1 = 0;
        if (!miss && S > 0) {
            const double a0 = floor(((double)tmin - (double)near) / (double)a.step - 0.5) - 2.0;
            const double a1 = floor(((double)tmax - (double)near) / (double)a.step - 0.5) + 3.0;
            i = (int)fmin(fmax(a0, 0.0), (double)S);
            i1 = (int)fmin(fmax(a1, 0.0), (double)S);
        }
        const float delta = a.step * nrm;
        const int cyc = a.R[1] - 1, czc = a.R[2] - 1;
        const int L = a.L, inm = (1 << L) - 1;
        // the brick this lane looked up last: its linear index, its slot and its exponent word (0 for an absent one)
        int last_key = -1, last_slot = -1;
        unsigned last_exp = 0u;
        float T = 1.f, img0 = 0.f, img1 = 0.f, img2 = 0.f, dep = 0.f, opa = 0.f;
        bool done = false;
        for (; i < i1 && !done; i += kBatch) {
            // which of the next kBatch samples have to be fetched: their occupancy words are loaded together (one latency, not kBatch)
            unsigned mask = 0;
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                int cj[3];
                float fj[3], tj;
                const bool need = i + k < i1 && locate(a, near, o3, d3, i + k, tj, cj, fj);
                const unsigned b = need ? ((unsigned)cj[0] * (unsigned)cyc + (unsigned)cj[1]) * (unsigned)czc + (unsigned)cj[2] : 0u;
                const unsigned word = a.skip ? a.bits[b >> 5] : 0xffffffffu;
                if (need && ((word >> (b & 31u)) & 1u)) mask |= 1u << k;
            }
            while (mask) {
            const int kk = __builtin_ctz(mask);
            mask &= mask - 1u;
            int ci[3];
            float fr[3], t;
            locate(a, near, o3, d3, i + kk, t, ci, fr);
            if (sub == 0) ++fetched;
            // the 8 corner records through the brick table, in front of the loads: at[cn] < 0 = a point of an absent brick
            int key[8], slot[8];
#pragma unroll
            for (int cn = 0; cn < 8; ++cn) {
                const int x = ci[0] + ((cn >> 2) & 1), y = ci[1] + ((cn >> 1) & 1), z = ci[2] + (cn & 1);
                key[cn] = ((x >> L) * a.By + (y >> L)) * a.Bz + (z >> L);
            }
#pragma unroll
            for (int cn = 0; cn < 8; ++cn) slot[cn] = key[cn] == last_key ? last_slot : a.brick_of[key[cn]];
            // a record's index fits 32 bits (n_bricks <= Bx By Bz, so at most 1032^3 records); its byte offset is formed in 64
            int at[8];
            unsigned ew[8];
#pragma unroll
            for (int cn = 0; cn < 8; ++cn) {
                const int x = ci[0] + ((cn >> 2) & 1), y = ci[1] + ((cn >> 1) & 1), z = ci[2] + (cn & 1);
                const int in = ((((x & inm) << L) | (y & inm)) << L) | (z & inm);
                const bool stored = slot[cn] >= 0 && (long long)slot[cn] < a.n_bricks;
                at[cn] = stored ? (int)(((unsigned)slot[cn] << (3 * L)) + (unsigned)in) : -1;
                // the brick's exponent word, by slot: it does not wait for the record
                ew[cn] = key[cn] == last_key ? last_exp : (stored ? a.exps[slot[cn]] : 0u);
            }
            last_key = key[0]; last_slot = slot[0]; last_exp = ew[0];
            float sig = 0.f, cf[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) cf[s] = 0.f;
#pragma unroll
            for (int cn = 0; cn < 8; ++cn) {
                const float w = ((cn & 4) ? fr[0] : 1.f - fr[0]) * ((cn & 2) ? fr[1] : 1.f - fr[1]) * ((cn & 1) ? fr[2] : 1.f - fr[2]);
                const long long pt = at[cn];                        // (sign-extended: -1 stays -1)
                unsigned wd[NW];
                if constexpr (NW == 2) {
                    const uint2 v = pt >= 0 ? *reinterpret_cast<const uint2*>(a.rec + pt * QB) : make_uint2(0u, 0u);
                    wd[0] = v.x; wd[1] = v.y;
                } else {
#pragma unroll
                    for (int j = 0; j < NW / 4; ++j) {
                        const uint4 v = pt >= 0 ? *reinterpret_cast<const uint4*>(a.rec + pt * QB + 16 * (G > 1 ? sub : j))
                                                : make_uint4(0u, 0u, 0u, 0u);
                        wd[4 * j] = v.x; wd[4 * j + 1] = v.y; wd[4 * j + 2] = v.z; wd[4 * j + 3] = v.w;
                    }
                }
                sig = __builtin_fmaf(w, (G == 1 || sub == 0) ? __uint_as_float(wd[0]) : 0.f, sig);      // byte 0..3 of the record
                if constexpr (G == 1) {
                    // this corner's scales, 2^e per band and -128 x each; every coefficient is decoded, then weighted
                    float sc[DEG + 1], ms[DEG + 1];
#pragma unroll
                    for (int l = 0; l <= DEG; ++l) {
                        sc[l] = band_scale(ew[cn], 8 * l);
                        ms[l] = __fmul_rn(sc[l], -128.f);
                    }
#pragma unroll
                    for (int e = 0; e < 3 * K; ++e) {
                        const unsigned x = wd[(4 + e) >> 2] ^ 0x80808080u;          // q + 128 in every byte
                        const float u = (float)((x >> (8 * ((4 + e) & 3))) & 0xffu);
                        const float c = __builtin_fmaf(u, sc[band_of(e)], ms[band_of(e)]);          // (u - 128) 2^e = q 2^e, exactly
                        cf[4 + e] = __builtin_fmaf(w, c, cf[4 + e]);
                    }
                } else {
                    // a group lane folds the scale of each of its three runs into the corner's weight: w 2^e is exact (short of
                    // underflow: w < 2^-102), so fma(q, w 2^e, acc) forms the same exact product w (q 2^e) as fma(w, q 2^e, acc) and
                    // rounds it once, like the decoded form -- one conversion and one fused multiply-add per byte
                    float ws[3];
#pragma unroll
                    for (int g = 0; g < 3; ++g) ws[g] = __fmul_rn(w, band_scale(ew[cn], sh[g]));
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const float qf = (float)((int)(wd[s >> 2] << (24 - 8 * (s & 3))) >> 24);    // the byte as a signed number
                        cf[s] = __builtin_fmaf(qf, ws[seg_of(s)], cf[s]);
                    }
                }
            }
            float col[3] = {0.f, 0.f, 0.f};
            if constexpr (G == 1) {
#pragma unroll
                for (int e = 0; e < 3 * K; ++e) col[e % 3] = __builtin_fmaf(cf[4 + e], Y[e / 3], col[e % 3]);
            } else {
                float part[3] = {0.f, 0.f, 0.f};                    // part[j]: the slots with (s + 2) mod 3 = j, channel (j + sub) mod 3
#pragma unroll
                for (int s = 0; s < NS; ++s) part[(s + 2) % 3] = __builtin_fmaf(cf[s], yk[s], part[(s + 2) % 3]);
                col[0] = rot == 0 ? part[0] : (rot == 1 ? part[2] : part[1]);
                col[1] = rot == 0 ? part[1] : (rot == 1 ? part[0] : part[2]);
                col[2] = rot == 0 ? part[2] : (rot == 1 ? part[1] : part[0]);
#pragma unroll
                for (int c = 0; c < 3; ++c) col[c] = group_sum<G>(col[c]);
                sig = group_first<G>(sig);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) col[c] = fminf(fmaxf(col[c], 0.f), 1.f);
            const float alpha = 1.f - expf(-(sig * delta));
            const float w = T * alpha;
            img0 = img0 + w * col[0]; img1 = img1 + w * col[1]; img2 = img2 + w * col[2];
            dep = dep + w * t;
            opa = opa + w;
            T = T * (1.f - alpha);
            if (a.eps > 0.f && T < a.eps) { done = true; break; }
            }
        }
        if (sub == 0) {
            if (a.image) {
                const float bg = a.white ? 1.f - opa : 0.f;
                a.image[ray * 3 + 0] = fminf(fmaxf(img0 + bg, 0.f), 1.f);
                a.image[ray * 3 + 1] = fminf(fmaxf(img1 + bg, 0.f), 1.f);
                a.image[ray * 3 + 2] = fminf(fmaxf(img2 + bg, 0.f), 1.f);
            }
            if (a.depth) a.depth[ray] = dep;
            if (a.opacity) a.opacity[ray] = opa;
        }
    }
    if (a.stats) {                                                  // every lane of the wave is back here: one atomic pair per wave
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            fetched += __shfl_down(fetched, off, 64);
            total += __shfl_down(total, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (fetched) atomicAdd(a.stats, fetched);
            if (total) atomicAdd(a.stats + 1, total);
        }
    }
}

template <int DEG, int G>
hipError_t launch_render(const RenderArgs& a, hipStream_t s) {
    const long long lanes = a.n * G, blocks = (lanes + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((baked_render_qbricks_kernel<DEG, G>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// what every entry point checks of the brick set behind its records: the refusals of knerf_baked_render_bricks.  B: the brick grid,
// scale: cells / (hi - lo) per axis
static bool check_bricks(const knerf_baked_bricks* f, int (&B)[3], float (&scale)[3]) {
    if (!f || !f->records) return false;
    // the unquantised record is the larger of the two: its bound covers both tables
    static_assert(rec_bytes(0) >= qrec_bytes(0) && rec_bytes(1) >= qrec_bytes(1) && rec_bytes(2) >= qrec_bytes(2) &&
                  rec_bytes(3) >= qrec_bytes(3), "the quantised record is the smaller one");
    unsigned long long points = 0;
    return check_lattice(f->resolution, f->lo, f->hi, f->sh_degree, scale, points) &&
           check_brick_grid(f->resolution, f->sh_degree, f->brick_log2, f->n_bricks, B);
}

// the group variant of each degree, which is also the one the library picks when the flags leave the choice to it: the fastest variant
// measured
constexpr int kQuantLaneGroups[4] = {1, 1, 2, 4};

static bool overlap(const void* p, unsigned long long np, const void* q, unsigned long long nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

}  // namespace quant
}  // namespace knerf

using namespace knerf;

extern "C" int knerf_baked_quantize_bricks(void* stream, const knerf_baked_bricks* src, void* dst_records, uint32_t* dst_exponents) {
    int B[3];
    float scale[3];
    if (!quant::check_bricks(src, B, scale) || !dst_records || !dst_exponents) return KNERF_ERR_INVALID;
    const int deg = src->sh_degree, L = src->brick_log2;
    const unsigned long long n_records = (unsigned long long)src->n_bricks << (3 * L);
    const unsigned long long src_bytes = n_records * (unsigned)baked::rec_bytes(deg), dst_bytes = n_records * (unsigned)quant::qrec_bytes(deg);
    if (quant::overlap(src->records, src_bytes, dst_records, dst_bytes)) return KNERF_ERR_INVALID;
    if (quant::overlap(src->records, src_bytes, dst_exponents, 4ull * src->n_bricks) ||
        quant::overlap(dst_records, dst_bytes, dst_exponents, 4ull * src->n_bricks)) return KNERF_ERR_INVALID;
    const uint4* s = static_cast<const uint4*>(src->records);
    unsigned* d = static_cast<unsigned*>(dst_records);
    const int places = 1 << (3 * L);
    const dim3 grid((unsigned)src->n_bricks), block((unsigned)(places < quant::kBlock ? places : quant::kBlock));
    hipStream_t st = (hipStream_t)stream;
    switch (deg) {
        case 0: hipLaunchKernelGGL(quant::baked_quantize_bricks_kernel<0>, grid, block, 0, st, s, d, dst_exponents, places); break;
        case 1: hipLaunchKernelGGL(quant::baked_quantize_bricks_kernel<1>, grid, block, 0, st, s, d, dst_exponents, places); break;
        case 2: hipLaunchKernelGGL(quant::baked_quantize_bricks_kernel<2>, grid, block, 0, st, s, d, dst_exponents, places); break;
        default: hipLaunchKernelGGL(quant::baked_quantize_bricks_kernel<3>, grid, block, 0, st, s, d, dst_exponents, places); break;
    }
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_dequantize_bricks(void* stream, const knerf_baked_qbricks* src, void* dst_records) {
    int B[3];
    float scale[3];
    if (!src || !src->exponents || !quant::check_bricks(&src->bricks, B, scale) || !dst_records) return KNERF_ERR_INVALID;
    const int deg = src->bricks.sh_degree, L = src->bricks.brick_log2;
    const unsigned long long n_records = (unsigned long long)src->bricks.n_bricks << (3 * L);
    const unsigned long long src_bytes = n_records * (unsigned)quant::qrec_bytes(deg), dst_bytes = n_records * (unsigned)baked::rec_bytes(deg);
    if (quant::overlap(src->bricks.records, src_bytes, dst_records, dst_bytes)) return KNERF_ERR_INVALID;
    if (quant::overlap(src->exponents, 4ull * src->bricks.n_bricks, dst_records, dst_bytes)) return KNERF_ERR_INVALID;
    const unsigned* s = static_cast<const unsigned*>(src->bricks.records);
    uint4* d = static_cast<uint4*>(dst_records);
    const dim3 grid((unsigned)((n_records + quant::kBlock - 1) / quant::kBlock)), block(quant::kBlock);
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)n_records;
    switch (deg) {
        case 0: hipLaunchKernelGGL(quant::baked_dequantize_bricks_kernel<0>, grid, block, 0, st, s, src->exponents, d, n, 3 * L); break;
        case 1: hipLaunchKernelGGL(quant::baked_dequantize_bricks_kernel<1>, grid, block, 0, st, s, src->exponents, d, n, 3 * L); break;
        case 2: hipLaunchKernelGGL(quant::baked_dequantize_bricks_kernel<2>, grid, block, 0, st, s, src->exponents, d, n, 3 * L); break;
        default: hipLaunchKernelGGL(quant::baked_dequantize_bricks_kernel<3>, grid, block, 0, st, s, src->exponents, d, n, 3 * L); break;
    }
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_render_qbricks(void* stream, const knerf_baked_qbricks* qfield, const float* origins, const float* directions,
                                          const float* near, const float* far, float near_all, float far_all, uint64_t n_rays, float step,
                                          float termination, int flags, float* image, float* depth, float* opacity, int64_t* stats) {
    if (!qfield || !qfield->exponents || !qfield->bricks.brick_of || !origins || !directions) return KNERF_ERR_INVALID;
    const knerf_baked_bricks* field = &qfield->bricks;
    quant::RenderArgs a{};
    int B[3];
    if (!quant::check_bricks(field, B, a.scale)) return KNERF_ERR_INVALID;
    if (!image && !depth && !opacity && !stats) return KNERF_ERR_INVALID;
    const int deg = field->sh_degree, L = field->brick_log2;
    if (!baked::check_rays(near, far, near_all, far_all, n_rays, step, termination, flags)) return KNERF_ERR_INVALID;
    if ((flags & KNERF_BAKED_SKIP_EMPTY) && !field->bits) return KNERF_ERR_INVALID;
    const int lanes = baked::pick_lanes(deg, flags, quant::kQuantLaneGroups);
    if (!lanes) return KNERF_ERR_INVALID;
    if (n_rays == 0) return KNERF_OK;
    for (int c = 0; c < 3; ++c) { a.R[c] = field->resolution[c]; a.lo[c] = field->lo[c]; a.hi[c] = field->hi[c]; }
    a.rec = static_cast<const unsigned char*>(field->records); a.exps = qfield->exponents; a.brick_of = field->brick_of; a.bits = field->bits;
    a.L = L; a.By = B[1]; a.Bz = B[2]; a.n_bricks = (long long)field->n_bricks;
    a.o = origins; a.d = directions; a.near = near; a.far = far; a.near0 = near_all; a.far0 = far_all;
    a.n = (long long)n_rays; a.step = step; a.eps = termination;
    a.white = (flags & KNERF_BAKED_WHITE_BACKGROUND) ? 1 : 0; a.skip = (flags & KNERF_BAKED_SKIP_EMPTY) ? 1 : 0;
    a.image = image; a.depth = depth; a.opacity = opacity; a.stats = reinterpret_cast<unsigned long long*>(stats);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipErrorInvalidValue;
    switch (deg * 8 + lanes) {
        case 0 * 8 + 1: e = quant::launch_render<0, 1>(a, s); break;
        case 1 * 8 + 1: e = quant::launch_render<1, 1>(a, s); break;
        case 2 * 8 + 1: e = quant::launch_render<2, 1>(a, s); break;
        case 2 * 8 + 2: e = quant::launch_render<2, 2>(a, s); break;
        case 3 * 8 + 1: e = quant::launch_render<3, 1>(a, s); break;
        case 3 * 8 + 4: e = quant::launch_render<3, 4>(a, s); break;
        default: return KNERF_ERR_INVALID;
    }
    return e == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
