// baked_query.hip -- what a baked field holds AT A POINT: density, colour along a direction and the density's gradient, for dense, brick
// and 8-bit brick storage (gfx950), context-free.  Extension: the reference has nothing of the kind (Plenoxels and PlenOctrees answer
// point queries on their grids and export meshes from them).  include/knerf.h (knerf_baked_query) holds the specification;
// tests/baked_query_reference.py restates it in fp64.  What the file shares with the other baked*.hip files (sh_eval, the DPP sums,
// the fp16 codec, the argument checks, the lane dispatch) is in baked_common.h.
//
// The evaluation is the one baked_render_kernel (baked.hip) makes of ONE sample, lifted out of the march: the cell lookup is locate
// without the ray, the corner order, the weights and every fused multiply-add are that kernel's text, so a queried sigma is the sigma
// the march composites at that position, and a queried colour is the colour it composites there.
//
//   baked_query_sigma_kernel <Args>          one point per lane, density (and gradient) only: it loads the FIRST WORD of each corner
//                          record, 4 bytes instead of 16 .. 112.  The record's size is a run-time stride, so the kernel serves every degree,
//                          and, through the brick argument struct, the 8-bit records as well (their first word is the same fp32 sigma).
//   baked_query_kernel <DEG, G, Args>        G lanes evaluate one point; lane `sub` of the group owns chunks sub, sub + G, ... of every
//                          corner record (G = 1: one point per lane; with G = record chunks the group reads each corner as ONE
//                          contiguous record).  The three channel sums are added across the group with the DPP quad permutes, sigma and
//                          the gradient come from the lane that owns chunk 0.  Args = QueryArgs (dense), BrickQueryArgs or
//                          QuantQueryArgs: ONE evaluation for the storages, only the record's address (Args::kBrick: through brick_of,
//                          with the range guard of the render) and its fetch (Args::kQuant: the 8-bit record, decoded to fp32 before
//                          fma(w, coeff, acc), the decode of baked_quant.hip) differ.  Dense and bricks give identical bits; the 8-bit
//                          records at one lane per point give the bits of the brick query on the dequantised records.
// No lane leaves early: a group whose point lies past n, or outside the box, goes through the evaluation on all-zero records without a
// memory access (every load is predicated on a valid address), so the lanes of a wave reach the DPP sums together; only the stores are
// skipped.
//
// Points come as a list [n,3] or are formed by the kernel from a grid spec, as knerf_query_grid places them:
// __fadd_rn(lo, __fmul_rn((float)idx, step)), step = (hi - lo) / (R - 1) in fp32, C order, z fastest.  No coordinate tensor exists.
#include "baked_common.h"

namespace knerf {
namespace bquery {
using namespace baked;

// ---- the 8-bit record and its decode: the text of baked_quant.hip (include/knerf.h knerf_baked_qbricks states the format)
constexpr int kExpMin = -24, kExpMax = 9;
__host__ __device__ constexpr int qrec_bytes(int deg) { return deg == 0 ? 8 : (deg == 1 ? 16 : (deg == 2 ? 32 : 64)); }
__host__ __device__ constexpr int band_of(int e) { return (e >= 3) + (e >= 12) + (e >= 27); }
__device__ __forceinline__ float pow2(int e) { return __int_as_float((e + 127) << 23); }
// 2^e of the exponent byte at bit `shift` of a brick's exponent word; a byte outside [-24, 9] (a damaged table) is clamped into it
__device__ __forceinline__ float band_scale(unsigned word, int shift) {
    int e = (int)((word >> shift) << 24) >> 24;
    e = e < kExpMin ? kExpMin : (e > kExpMax ? kExpMax : e);
    return pow2(e);
}
// a group lane's 16 bytes fall into three runs inside each of which every coefficient slot has one band (baked_quant.hip)
__host__ __device__ constexpr int seg_of(int s) { return s < 7 ? 0 : (s < 15 ? 1 : 2); }
__host__ __device__ constexpr int seg_first(int g) { return g == 0 ? 4 : (g == 1 ? 7 : 15); }
constexpr int kQuantLaneGroups[4] = {1, 1, 2, 4};

// ---- arguments.  Points: what is evaluated and where the results go, the same fields in every argument struct
struct Points {
    const float* pts;                               // [n,3], or nullptr in grid mode
    const float* dir;                               // nullptr, [3] or [n,3]
    int per_point, grid;
    int G[3];                                       // grid mode: the grid's resolution, its lower corner and its fp32 step
    float glo[3], gstep[3];
    long long n;
    float *sigma, *rgb, *grad;
};
struct QueryArgs : Points {
    static constexpr bool kBrick = false, kQuant = false;
    const uint4* rec;
    int rec_words;                                  // 4-byte words per record (the sigma-only kernel's stride)
    int R[3];
    float lo[3], scale[3];
};
struct BrickQueryArgs : Points {
    static constexpr bool kBrick = true, kQuant = false;
    const uint4* rec;
    int rec_words;
    const int* brick_of;
    int R[3];
    int L, By, Bz;                                  // log2 of the brick edge; the brick grid's y and z extents
    long long n_bricks;
    float lo[3], scale[3];
};
struct QuantQueryArgs : Points {
    static constexpr bool kBrick = true, kQuant = true;
    const unsigned char* rec;
    const unsigned* exps;
    const int* brick_of;
    int R[3];
    int L, By, Bz;
    long long n_bricks;
    float lo[3], scale[3];
};

// point `pt` of the list or of the grid, and, if it lies inside the field's box (the return value), its cell and the trilinear
// fractions: locate (baked_common.h) without the ray.  A NaN coordinate fails both comparisons: outside.  The cell index stays in range
// on every axis whatever u is.
template <class Args>
__device__ __forceinline__ bool locate_point(const Args& a, long long pt, int (&ci)[3], float (&fr)[3]) {
    float p[3];
    if (a.grid) {
        const long long yz = (long long)a.G[1] * a.G[2];
        const long long i = pt / yz, r = pt - i * yz, j = r / a.G[2], k = r - j * a.G[2];
        p[0] = __fadd_rn(a.glo[0], __fmul_rn((float)i, a.gstep[0]));
        p[1] = __fadd_rn(a.glo[1], __fmul_rn((float)j, a.gstep[1]));
        p[2] = __fadd_rn(a.glo[2], __fmul_rn((float)k, a.gstep[2]));
    } else {
        p[0] = a.pts[pt * 3 + 0]; p[1] = a.pts[pt * 3 + 1]; p[2] = a.pts[pt * 3 + 2];
    }
    bool inside = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float u = __fmul_rn(__fsub_rn(p[c], a.lo[c]), a.scale[c]);
        const int cells = a.R[c] - 1;
        const bool in = u >= 0.f && u <= (float)cells;
        inside = inside && in;
        const int f = in ? (int)__builtin_floorf(u) : 0;
        ci[c] = f < cells ? f : cells - 1;
        fr[c] = __fsub_rn(u, (float)ci[c]);
    }
    return inside;
}

// the 8 corner records of a cell: at[cn] = the record's index, -1 for a record that reads as all-zero (a point of an absent brick, a
// brick_of value outside [0, n_bricks), and every corner of a point that is not evaluated: nothing is loaded for those).  ew[cn]: the
// exponent word of the corner's brick (8-bit storage)
template <class Args>
__device__ __forceinline__ void corner_records(const Args& a, bool inside, const int (&ci)[3], long long (&at)[8], unsigned (&ew)[8]) {
    if constexpr (!Args::kBrick) {
        const long long sy = a.R[2], sx = (long long)a.R[1] * a.R[2];
        const long long base = (long long)ci[0] * sx + (long long)ci[1] * sy + ci[2];
#pragma unroll
        for (int cn = 0; cn < 8; ++cn) {
            at[cn] = inside ? base + ((cn & 4) ? sx : 0) + ((cn & 2) ? sy : 0) + (cn & 1) : -1;
            ew[cn] = 0u;
        }
    } else {
        const int L = a.L, inm = (1 << L) - 1;
        int slot[8];
#pragma unroll
        for (int cn = 0; cn < 8; ++cn) {
            const int x = ci[0] + ((cn >> 2) & 1), y = ci[1] + ((cn >> 1) & 1), z = ci[2] + (cn & 1);
            slot[cn] = inside ? a.brick_of[((x >> L) * a.By + (y >> L)) * a.Bz + (z >> L)] : -1;
        }
#pragma unroll
        for (int cn = 0; cn < 8; ++cn) {
            const int x = ci[0] + ((cn >> 2) & 1), y = ci[1] + ((cn >> 1) & 1), z = ci[2] + (cn & 1);
            const int in = ((((x & inm) << L) | (y & inm)) << L) | (z & inm);
            const bool stored = slot[cn] >= 0 && (long long)slot[cn] < a.n_bricks;
            at[cn] = stored ? ((long long)slot[cn] << (3 * L)) + in : -1;
            if constexpr (Args::kQuant) ew[cn] = stored ? a.exps[slot[cn]] : 0u; else ew[cn] = 0u;
        }
    }
}

// corner cn = 0..7 has x = bit 2, y = bit 1, z = bit 0: the weights of baked_render_kernel
__device__ __forceinline__ void corner_weights(const float (&fr)[3], float (&w)[8]) {
#pragma unroll
    for (int cn = 0; cn < 8; ++cn)
        w[cn] = ((cn & 4) ? fr[0] : 1.f - fr[0]) * ((cn & 2) ? fr[1] : 1.f - fr[1]) * ((cn & 1) ? fr[2] : 1.f - fr[2]);
}

__device__ __forceinline__ float corner_sigma(const float (&w)[8], const float (&sg)[8]) {
    float sig = 0.f;
#pragma unroll
    for (int cn = 0; cn < 8; ++cn) sig = __builtin_fmaf(w[cn], sg[cn], sig);
    return sig;
}

// the exact gradient of the trilinear sigma inside the located cell: per axis the four corner pairs (lower corner in ascending order)
// weighted with the other two axes' weights, one fused multiply-add each, then one multiply by the axis' scale
__device__ __forceinline__ void sigma_gradient(const float (&fr)[3], const float (&sg)[8], const float (&scale)[3], float (&g)[3]) {
    const float f0[3] = {1.f - fr[0], 1.f - fr[1], 1.f - fr[2]};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int bit = 4 >> ax, b = ax == 0 ? 1 : 0, c = ax == 2 ? 1 : 2;       // the other two axes, x before y before z
        float s = 0.f;
#pragma unroll
        for (int cn = 0; cn < 8; ++cn) {
            if (cn & bit) continue;
            const float wb = (cn & (4 >> b)) ? fr[b] : f0[b], wc = (cn & (4 >> c)) ? fr[c] : f0[c];
            s = __builtin_fmaf(wb * wc, sg[cn | bit] - sg[cn], s);
        }
        g[ax] = s * scale[ax];
    }
}

// ---- density (and gradient) only
template <class Args>
__global__ __launch_bounds__(kBlock) void baked_query_sigma_kernel(Args a) {
    static_assert(!Args::kQuant, "the 8-bit records go through the brick arguments: their first word is the same sigma");
    const long long pt = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (pt >= a.n) return;
    int ci[3];
    float fr[3];
    const bool inside = locate_point(a, pt, ci, fr);
    long long at[8];
    unsigned ew[8];
    corner_records(a, inside, ci, at, ew);
    const unsigned* words = reinterpret_cast<const unsigned*>(a.rec);
    float sg[8], w[8];
#pragma unroll
    for (int cn = 0; cn < 8; ++cn) sg[cn] = at[cn] >= 0 ? __uint_as_float(words[at[cn] * a.rec_words]) : 0.f;
    corner_weights(fr, w);
    if (a.sigma) a.sigma[pt] = inside ? corner_sigma(w, sg) : 0.f;
    if (a.grad) {
        float g[3];
        sigma_gradient(fr, sg, a.scale, g);
        a.grad[pt * 3 + 0] = inside ? g[0] : 0.f; a.grad[pt * 3 + 1] = inside ? g[1] : 0.f; a.grad[pt * 3 + 2] = inside ? g[2] : 0.f;
    }
}

// ---- the corner sums of a lane: sg[cn] = the corner's sigma (0 on a lane that does not own chunk 0), col = this lane's share of the
// three channel sums

// fp16 records (dense and bricks): the text of baked_render_kernel
template <int DEG, int G, class Args>
__device__ __forceinline__ void corner_sums(const Args& a, const long long (&at)[8], const float (&w)[8], const float (&Y)[n_coeff(DEG)],
                                            int sub, float (&sg)[8], float (&col)[3]) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, CPL = (NCH + G - 1) / G;     // chunks per record / per lane
    float cf[CPL][8];
#pragma unroll
    for (int j = 0; j < CPL; ++j)
#pragma unroll
        for (int s = 0; s < 8; ++s) cf[j][s] = 0.f;
#pragma unroll
    for (int cn = 0; cn < 8; ++cn) {
        uint4 v[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int qc = sub + j * G;
            v[j] = (qc < NCH && at[cn] >= 0) ? a.rec[at[cn] * NCH + qc] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const unsigned wd[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            if (j == 0) sg[cn] = sub == 0 ? __uint_as_float(wd[0]) : 0.f;      // chunk 0: its first word is sigma, not two halfs
#pragma unroll
            for (int s = 0; s < 8; ++s) cf[j][s] = __builtin_fmaf(w[cn], half_bits_to_float(wd[s >> 1] >> ((s & 1) * 16)), cf[j][s]);
        }
    }
    // slots that hold no coefficient (sigma's two in chunk 0, the padding behind 3 K halfs, chunks past the record) count as 0
    // whatever their bits are: a record's padding is never trusted
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int e = 8 * (sub + j * G) - 2 + s;
            cf[j][s] = (e >= 0 && e < 3 * K) ? cf[j][s] : 0.f;
        }
    }
    col[0] = col[1] = col[2] = 0.f;
    if constexpr (G == 1) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int e = 8 * j - 2 + s;
                if (e >= 0 && e < 3 * K) col[e % 3] = __builtin_fmaf(cf[j][s], Y[e / 3], col[e % 3]);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                // which basis value and channel this half slot carries: 0 for a slot that holds no coefficient
                const int e = 8 * (sub + j * G) - 2 + s;
                const int k = e / 3, c = e - 3 * k;
                float yk = 0.f;
#pragma unroll
                for (int kk = 0; kk < K; ++kk) yk = (e >= 0 && k == kk) ? Y[kk] : yk;
                col[0] = __builtin_fmaf(cf[j][s], c == 0 ? yk : 0.f, col[0]);
                col[1] = __builtin_fmaf(cf[j][s], c == 1 ? yk : 0.f, col[1]);
                col[2] = __builtin_fmaf(cf[j][s], c == 2 ? yk : 0.f, col[2]);
            }
        }
    }
}

// 8-bit records: the text of baked_render_qbricks_kernel.  G = 1 decodes every coefficient to fp32 and accumulates in ascending
// e = 3 k + c, as corner_sums<DEG, 1> does on the dequantised record; a group lane takes one 16-byte chunk and folds the power of two
// into the corner's weight (w 2^e is exact short of underflow, so the fused multiply-add rounds the same exact product once)
template <int DEG, int G>
__device__ __forceinline__ void corner_sums_quant(const QuantQueryArgs& a, const long long (&at)[8], const unsigned (&ew)[8],
                                                  const float (&w)[8], const float (&Y)[n_coeff(DEG)], int sub, float (&sg)[8],
                                                  float (&col)[3]) {
    constexpr int K = n_coeff(DEG), QB = qrec_bytes(DEG), NW = QB / 4 / G, NS = 4 * NW;     // words / byte slots of a record per lane
    static_assert(G == 1 || (G == 2 && DEG == 2) || (G == 4 && DEG == 3), "a group takes one 16-byte chunk per lane");
    static_assert(G == 1 || NW == 4, "a group takes one 16-byte chunk per lane");
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
            sh[g] = 8 * (l < DEG ? l : DEG);                        // (a run of padding only: any band the degree has)
        }
        rot = sub % 3;
    }
    float cf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) cf[s] = 0.f;
#pragma unroll
    for (int cn = 0; cn < 8; ++cn) {
        const long long pt = at[cn];
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
        sg[cn] = (G == 1 || sub == 0) ? __uint_as_float(wd[0]) : 0.f;           // bytes 0..3 of the record
        if constexpr (G == 1) {
            float sc[DEG + 1], ms[DEG + 1];
#pragma unroll
            for (int l = 0; l <= DEG; ++l) {
                sc[l] = band_scale(ew[cn], 8 * l);
                ms[l] = __fmul_rn(sc[l], -128.f);
            }
#pragma unroll
            for (int e = 0; e < 3 * K; ++e) {
                const unsigned x = wd[(4 + e) >> 2] ^ 0x80808080u;              // q + 128 in every byte
                const float u = (float)((x >> (8 * ((4 + e) & 3))) & 0xffu);
                const float c = __builtin_fmaf(u, sc[band_of(e)], ms[band_of(e)]);          // (u - 128) 2^e = q 2^e, exactly
                cf[4 + e] = __builtin_fmaf(w[cn], c, cf[4 + e]);
            }
        } else {
            float ws[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) ws[g] = __fmul_rn(w[cn], band_scale(ew[cn], sh[g]));
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float qf = (float)((int)(wd[s >> 2] << (24 - 8 * (s & 3))) >> 24);    // the byte as a signed number
                cf[s] = __builtin_fmaf(qf, ws[seg_of(s)], cf[s]);
            }
        }
    }
    col[0] = col[1] = col[2] = 0.f;
    if constexpr (G == 1) {
#pragma unroll
        for (int e = 0; e < 3 * K; ++e) col[e % 3] = __builtin_fmaf(cf[4 + e], Y[e / 3], col[e % 3]);
    } else {
        float part[3] = {0.f, 0.f, 0.f};                            // part[j]: the slots with (s + 2) mod 3 = j, channel (j + sub) mod 3
#pragma unroll
        for (int s = 0; s < NS; ++s) part[(s + 2) % 3] = __builtin_fmaf(cf[s], yk[s], part[(s + 2) % 3]);
        col[0] = rot == 0 ? part[0] : (rot == 1 ? part[2] : part[1]);
        col[1] = rot == 0 ? part[1] : (rot == 1 ? part[0] : part[2]);
        col[2] = rot == 0 ? part[2] : (rot == 1 ? part[1] : part[0]);
    }
}

// ---- density, colour and gradient
template <int DEG, int G, class Args>
__global__ __launch_bounds__(kBlock) void baked_query_kernel(Args a) {
    constexpr int K = n_coeff(DEG);
    static_assert(G == 1 || G == 2 || G == 4, "a group is a lane, a pair or a quad");
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long pt = gid / G;
    const int sub = (int)(gid & (G - 1));
    const bool have = pt < a.n;                                     // the same for every lane of a group
    int ci[3] = {0, 0, 0};
    float fr[3] = {0.f, 0.f, 0.f};
    bool inside = false;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (have) {
        inside = locate_point(a, pt, ci, fr);
        if (a.dir) {
            const float* d = a.dir + (a.per_point ? pt * 3 : 0);
            dx = d[0]; dy = d[1]; dz = d[2];
        }
    }
    long long at[8];
    unsigned ew[8];
    corner_records(a, inside, ci, at, ew);
    // the direction, normalised as the render normalises d; none, or one whose length is 0 or not finite: the DC term alone
    const float nrm = __fsqrt_rn(dx * dx + dy * dy + dz * dz);
    const bool seen = nrm > 0.f && nrm < INFINITY;
    const float ux = seen ? dx / nrm : 0.f, uy = seen ? dy / nrm : 0.f, uz = seen ? dz / nrm : 0.f;
    float Y[K];
    sh_eval<DEG>(ux, uy, uz, Y);
#pragma unroll
    for (int k = 1; k < K; ++k) Y[k] = seen ? Y[k] : 0.f;
    float w[8], sg[8], col[3];
    corner_weights(fr, w);
    if constexpr (Args::kQuant) corner_sums_quant<DEG, G>(a, at, ew, w, Y, sub, sg, col);
    else corner_sums<DEG, G>(a, at, w, Y, sub, sg, col);
    if constexpr (G > 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) col[c] = group_sum<G>(col[c]);  // every lane of the wave is here
    }
    if (!have || sub != 0) return;
    if (a.sigma) a.sigma[pt] = inside ? corner_sigma(w, sg) : 0.f;
    if (a.rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.rgb[pt * 3 + c] = inside ? fminf(fmaxf(col[c], 0.f), 1.f) : 0.f;
    }
    if (a.grad) {
        float g[3];
        sigma_gradient(fr, sg, a.scale, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.grad[pt * 3 + c] = inside ? g[c] : 0.f;
    }
}

// ---- host
template <class Args>
static hipError_t launch_sigma(const Args& a, hipStream_t s) {
    const long long blocks = (a.n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((baked_query_sigma_kernel<Args>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

template <int DEG, int G, class Args>
static hipError_t launch_full(const Args& a, hipStream_t s) {
    const long long blocks = (a.n * G + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((baked_query_kernel<DEG, G, Args>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// what every entry point checks of its query; p and lanes come back resolved.  n = 0 is for the caller
static bool check_query(const knerf_baked_query_spec* q, int deg, const int (&group)[4], Points& p, int& lanes) {
    if (!q) return false;
    if (!q->sigma && !q->rgb && !q->gradient) return false;
    const bool grid = q->grid_resolution || q->grid_lo || q->grid_hi;
    if (grid == (q->points != nullptr)) return false;                           // neither, or both
    if (q->flags & ~KNERF_BAKED_LANES_MASK) return false;
    if (q->per_point != 0 && q->per_point != 1) return false;
    lanes = pick_lanes(deg, q->flags, group);
    if (!lanes) return false;
    unsigned long long n = q->n;
    if (grid) {
        if (!q->grid_resolution || !q->grid_lo || !q->grid_hi) return false;
        n = 1;
        for (int c = 0; c < 3; ++c) {
            const int r = q->grid_resolution[c];
            const float l = q->grid_lo[c], h = q->grid_hi[c];
            if (r < 2) return false;
            if (!std::isfinite(l) || !std::isfinite(h) || !(h > l)) return false;
            const float step = (h - l) / (float)(r - 1);                        // fp32 subtraction and division, as knerf_query_grid
            if (!std::isfinite(step)) return false;
            n *= (unsigned)r;
            if (n > (1ull << 31)) return false;
            p.G[c] = r; p.glo[c] = l; p.gstep[c] = step;
        }
    }
    if (n >= (1ull << 36)) return false;
    p.pts = q->points; p.dir = q->directions; p.per_point = q->per_point; p.grid = grid ? 1 : 0; p.n = (long long)n;
    p.sigma = q->sigma; p.rgb = q->rgb; p.grad = q->gradient;
    return true;
}

template <class Args>
static void set_lattice(Args& a, const int32_t* resolution, const float* lo) {
    for (int c = 0; c < 3; ++c) { a.R[c] = resolution[c]; a.lo[c] = lo[c]; }
}

}  // namespace bquery
}  // namespace knerf

using namespace knerf;

extern "C" int knerf_baked_query(void* stream, const knerf_baked_field* field, const knerf_baked_query_spec* query) {
    if (!field || !field->records) return KNERF_ERR_INVALID;
    bquery::QueryArgs a{};
    unsigned long long points = 0;
    int lanes = 0;
    const int deg = field->sh_degree;
    if (!baked::check_lattice(field->resolution, field->lo, field->hi, deg, a.scale, points)) return KNERF_ERR_INVALID;
    if (!bquery::check_query(query, deg, baked::kLaneGroups, a, lanes)) return KNERF_ERR_INVALID;
    if (a.n == 0) return KNERF_OK;
    bquery::set_lattice(a, field->resolution, field->lo);
    a.rec = static_cast<const uint4*>(field->records); a.rec_words = baked::rec_bytes(deg) / 4;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = !a.rgb ? bquery::launch_sigma(a, s) : baked::dispatch_deg_lanes(deg, lanes, [&](auto DEG, auto G) {
        return bquery::launch_full<DEG, G>(a, s);
    });
    return e == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_query_bricks(void* stream, const knerf_baked_bricks* field, const knerf_baked_query_spec* query) {
    if (!field || !field->records || !field->brick_of) return KNERF_ERR_INVALID;
    bquery::BrickQueryArgs a{};
    unsigned long long points = 0;
    int lanes = 0, B[3];
    const int deg = field->sh_degree;
    if (!baked::check_lattice(field->resolution, field->lo, field->hi, deg, a.scale, points)) return KNERF_ERR_INVALID;
    if (!baked::check_brick_grid(field->resolution, deg, field->brick_log2, field->n_bricks, B)) return KNERF_ERR_INVALID;
    if (!bquery::check_query(query, deg, baked::kLaneGroups, a, lanes)) return KNERF_ERR_INVALID;
    if (a.n == 0) return KNERF_OK;
    bquery::set_lattice(a, field->resolution, field->lo);
    a.rec = static_cast<const uint4*>(field->records); a.rec_words = baked::rec_bytes(deg) / 4; a.brick_of = field->brick_of;
    a.L = field->brick_log2; a.By = B[1]; a.Bz = B[2]; a.n_bricks = (long long)field->n_bricks;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = !a.rgb ? bquery::launch_sigma(a, s) : baked::dispatch_deg_lanes(deg, lanes, [&](auto DEG, auto G) {
        return bquery::launch_full<DEG, G>(a, s);
    });
    return e == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_query_qbricks(void* stream, const knerf_baked_qbricks* qfield, const knerf_baked_query_spec* query) {
    if (!qfield || !qfield->exponents || !qfield->bricks.records || !qfield->bricks.brick_of) return KNERF_ERR_INVALID;
    const knerf_baked_bricks* field = &qfield->bricks;
    bquery::QuantQueryArgs a{};
    unsigned long long points = 0;
    int lanes = 0, B[3];
    const int deg = field->sh_degree;
    // the unquantised record is the larger of the two: its bound covers both tables
    if (!baked::check_lattice(field->resolution, field->lo, field->hi, deg, a.scale, points)) return KNERF_ERR_INVALID;
    if (!baked::check_brick_grid(field->resolution, deg, field->brick_log2, field->n_bricks, B)) return KNERF_ERR_INVALID;
    if (!bquery::check_query(query, deg, bquery::kQuantLaneGroups, a, lanes)) return KNERF_ERR_INVALID;
    if (a.n == 0) return KNERF_OK;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipErrorInvalidValue;
    if (!a.rgb) {
        // density and gradient: the brick kernel on the 8-bit records, whose first word is the fp32 sigma
        bquery::BrickQueryArgs b{};
        static_cast<bquery::Points&>(b) = a;
        bquery::set_lattice(b, field->resolution, field->lo);
        for (int c = 0; c < 3; ++c) b.scale[c] = a.scale[c];
        b.rec = static_cast<const uint4*>(field->records); b.rec_words = bquery::qrec_bytes(deg) / 4; b.brick_of = field->brick_of;
        b.L = field->brick_log2; b.By = B[1]; b.Bz = B[2]; b.n_bricks = (long long)field->n_bricks;
        e = bquery::launch_sigma(b, s);
        return e == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
    }
    bquery::set_lattice(a, field->resolution, field->lo);
    a.rec = static_cast<const unsigned char*>(field->records); a.exps = qfield->exponents; a.brick_of = field->brick_of;
    a.L = field->brick_log2; a.By = B[1]; a.Bz = B[2]; a.n_bricks = (long long)field->n_bricks;
    switch (deg * 8 + lanes) {
        case 0 * 8 + 1: e = bquery::launch_full<0, 1>(a, s); break;
        case 1 * 8 + 1: e = bquery::launch_full<1, 1>(a, s); break;
        case 2 * 8 + 1: e = bquery::launch_full<2, 1>(a, s); break;
        case 2 * 8 + 2: e = bquery::launch_full<2, 2>(a, s); break;
        case 3 * 8 + 1: e = bquery::launch_full<3, 1>(a, s); break;
        case 3 * 8 + 4: e = bquery::launch_full<3, 4>(a, s); break;
        default: return KNERF_ERR_INVALID;
    }
    return e == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
