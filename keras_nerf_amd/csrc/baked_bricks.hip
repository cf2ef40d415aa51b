// baked_bricks.hip -- the baked field stored as sparse bricks, and its renderer (gfx950), context-free.
// Extension: the reference has nothing of the kind (PlenOctrees, SNeRG's macroblock atlas and Plenoxels store only the occupied part of
// their grids behind a coarse index).
//
// The lattice [Rx][Ry][Rz] of baked.hip is cut into BRICKS of b^3 lattice points, b = 1 << brick_log2 = 4 or 8: point (x, y, z) lies in
// brick (x >> L, y >> L, z >> L) of the brick grid B_a = ceil(R_a / b), at place ((x & (b-1)) b + (y & (b-1))) b + (z & (b-1)) in it.
//   brick_of  int32 [Bx][By][Bz]: the slot of a stored brick, -1 for an absent one
//   records   [n_bricks][b^3] records in the layout of baked.hip (fp32 sigma, 3 K halfs [k][c], zero padding to 16 bytes)
// A point of an absent brick reads as an all-zero record.  A brick_of value outside [0, n_bricks) counts as absent: a damaged table
// never becomes an out-of-range read.  The occupancy bits are those of the dense field.
//
//   baked_render_bricks_kernel  <DEG, G>: the march of baked_render_kernel (baked.hip) restated word for word -- sample positions,
//                          locate, corner order, the fused multiply-adds, lane variants, DPP group sums, batches of kBatch occupancy
//                          words, termination, stats -- so that every sample's arithmetic is the dense kernel's and the outputs are
//                          bit-identical (tests/test_gpu_baked_bricks.py holds the two in step).  Only the record address differs: the
//                          8 corner addresses are formed through brick_of in front of the record loads, so the loads still issue
//                          together (the march is bound by memory latency).  Each lane keeps the brick it looked up last (linear brick
//                          index and slot): consecutive samples mostly stay in one brick, and with b = 8 about two thirds of the
//                          samples have all 8 corners in one, so most samples need no table read at all.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/knerf.h"

namespace knerf {
namespace bricks {

constexpr int kBlock = 256;
constexpr int kBatch = 8;                           // samples whose occupancy bits are looked up together
constexpr int kMaxSamples = 1 << 23;               // (float)i + 0.5f is exact below this
constexpr unsigned long long kMaxBytes = 1ull << 40;

__host__ __device__ constexpr int n_coeff(int deg) { return (deg + 1) * (deg + 1); }
__host__ __device__ constexpr int rec_bytes(int deg) { return (4 + 6 * n_coeff(deg) + 15) / 16 * 16; }

__device__ __forceinline__ float half_bits_to_float(unsigned h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(h & 0xffffu)); }

struct RenderArgs {
    const uint4* rec;
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

// the orthonormal real spherical harmonics of a unit vector, index k = l (l + 1) + m, no Condon-Shortley phase
template <int DEG>
__device__ __forceinline__ void sh_eval(float x, float y, float z, float (&Y)[n_coeff(DEG)]) {
    Y[0] = 0.28209479177387814f;
    if constexpr (DEG >= 1) {
        Y[1] = 0.4886025119029199f * y;
        Y[2] = 0.4886025119029199f * z;
        Y[3] = 0.4886025119029199f * x;
    }
    if constexpr (DEG >= 2) {
        const float xx = x * x, yy = y * y, zz = z * z;
        Y[4] = 1.0925484305920792f * (x * y);
        Y[5] = 1.0925484305920792f * (y * z);
        Y[6] = 0.31539156525252005f * (3.f * zz - 1.f);
        Y[7] = 1.0925484305920792f * (x * z);
        Y[8] = 0.5462742152960396f * (xx - yy);
        if constexpr (DEG >= 3) {
            Y[9] = 0.5900435899266435f * (y * (3.f * xx - yy));
            Y[10] = 2.890611442640554f * (x * y * z);
            Y[11] = 0.4570457994644658f * (y * (5.f * zz - 1.f));
            Y[12] = 0.3731763325901154f * (z * (5.f * zz - 3.f));
            Y[13] = 0.4570457994644658f * (x * (5.f * zz - 1.f));
            Y[14] = 1.445305721320277f * (z * (xx - yy));
            Y[15] = 0.5900435899266435f * (x * (xx - 3.f * yy));
        }
    }
}

template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
// sum over the G lanes of a group (G = 2: lane pairs, G = 4: quads); every lane ends with the same bits
template <int G>
__device__ __forceinline__ float group_sum(float x) {
    if constexpr (G >= 2) x = x + dpp<0xB1>(x);        // quad_perm [1,0,3,2]
    if constexpr (G >= 4) x = x + dpp<0x4E>(x);        // quad_perm [2,3,0,1]
    return x;
}
template <int G>
__device__ __forceinline__ float group_first(float x) {
    if constexpr (G == 2) return dpp<0xA0>(x);         // quad_perm [0,0,2,2]
    if constexpr (G == 4) return dpp<0x00>(x);         // quad_perm [0,0,0,0]
    return x;
}

// sample i of a ray: t_i, and if the sample lies inside the box (the return value) its cell and the trilinear fractions
__device__ __forceinline__ bool locate(const RenderArgs& a, float near, const float (&o3)[3], const float (&d3)[3], int i, float& t,
                                       int (&ci)[3], float (&fr)[3]) {
    t = __fadd_rn(near, __fmul_rn((float)i + 0.5f, a.step));
    bool inside = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float p = __fadd_rn(o3[c], __fmul_rn(d3[c], t));
        const float u = __fmul_rn(__fsub_rn(p, a.lo[c]), a.scale[c]);
        const int cells = a.R[c] - 1;
        const bool in = u >= 0.f && u <= (float)cells;
        inside = inside && in;
        const int f = in ? (int)__builtin_floorf(u) : 0;
        ci[c] = f < cells ? f : cells - 1;
        fr[c] = __fsub_rn(u, (float)ci[c]);
    }
    return inside;
}

template <int DEG, int G>
__global__ __launch_bounds__(kBlock) void baked_render_bricks_kernel(RenderArgs a) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, CPL = (NCH + G - 1) / G;     // chunks per record / per lane
    static_assert(G == 1 || G == 2 || G == 4, "a group is a lane, a pair or a quad");
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
        // G > 1: which basis value and channel each of this lane's half slots carries (constant along the ray)
        float wr[CPL][8], wg[CPL][8], wb[CPL][8];
        if constexpr (G > 1) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int e = 8 * (sub + j * G) - 2 + s;
                    const int k = e / 3, c = e - 3 * k;
                    float yk = 0.f;
#pragma unroll
                    for (int kk = 0; kk < K; ++kk) yk = (e >= 0 && k == kk) ? Y[kk] : yk;
                    wr[j][s] = c == 0 ? yk : 0.f; wg[j][s] = c == 1 ? yk : 0.f; wb[j][s] = c == 2 ? yk : 0.f;
                }
            }
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
        // the brick this lane looked up last.  (One entry per corner was measured too: 26 more VGPRs, a wave per SIMD fewer, 9 % slower.)
        int last_key = -1, last_slot = -1;
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
            last_key = key[0]; last_slot = slot[0];
            // a record's index fits 32 bits (n_bricks <= Bx By Bz, so at most 1032^3 records); its byte offset is formed in 64
            int at[8];
#pragma unroll
            for (int cn = 0; cn < 8; ++cn) {
                const int x = ci[0] + ((cn >> 2) & 1), y = ci[1] + ((cn >> 1) & 1), z = ci[2] + (cn & 1);
                const int in = ((((x & inm) << L) | (y & inm)) << L) | (z & inm);
                const bool stored = slot[cn] >= 0 && (long long)slot[cn] < a.n_bricks;
                at[cn] = stored ? (int)(((unsigned)slot[cn] << (3 * L)) + (unsigned)in) : -1;
            }
            float sig = 0.f, cf[CPL][8];
#pragma unroll
            for (int j = 0; j < CPL; ++j)
#pragma unroll
                for (int s = 0; s < 8; ++s) cf[j][s] = 0.f;
#pragma unroll
            for (int cn = 0; cn < 8; ++cn) {
                const float w = ((cn & 4) ? fr[0] : 1.f - fr[0]) * ((cn & 2) ? fr[1] : 1.f - fr[1]) * ((cn & 1) ? fr[2] : 1.f - fr[2]);
                const long long pt = at[cn];                        // (sign-extended: -1 stays -1)
                uint4 v[CPL];
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const int qc = sub + j * G;
                    v[j] = (qc < NCH && pt >= 0) ? a.rec[pt * NCH + qc] : make_uint4(0u, 0u, 0u, 0u);
                }
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const unsigned wd[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                    const bool first = j == 0 && sub == 0;          // chunk 0: its first word is sigma, not two halfs
                    if (j == 0) sig = __builtin_fmaf(w, first ? __uint_as_float(wd[0]) : 0.f, sig);
#pragma unroll
                    for (int s = 0; s < 8; ++s) {
                        cf[j][s] = __builtin_fmaf(w, half_bits_to_float(wd[s >> 1] >> ((s & 1) * 16)), cf[j][s]);
                    }
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
            float col[3] = {0.f, 0.f, 0.f};
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
                        col[0] = __builtin_fmaf(cf[j][s], wr[j][s], col[0]);
                        col[1] = __builtin_fmaf(cf[j][s], wg[j][s], col[1]);
                        col[2] = __builtin_fmaf(cf[j][s], wb[j][s], col[2]);
                    }
                }
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
    hipLaunchKernelGGL((baked_render_bricks_kernel<DEG, G>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace bricks
}  // namespace knerf

using namespace knerf;

extern "C" int knerf_baked_render_bricks(void* stream, const knerf_baked_bricks* field, const float* origins, const float* directions,
                                         const float* near, const float* far, float near_all, float far_all, uint64_t n_rays, float step,
                                         float termination, int flags, float* image, float* depth, float* opacity, int64_t* stats) {
    if (!field || !field->records || !field->brick_of || !origins || !directions) return KNERF_ERR_INVALID;
    if (!image && !depth && !opacity && !stats) return KNERF_ERR_INVALID;
    const int deg = field->sh_degree;
    if (deg < 0 || deg > 3) return KNERF_ERR_INVALID;
    if (flags & ~(KNERF_BAKED_WHITE_BACKGROUND | KNERF_BAKED_SKIP_EMPTY | KNERF_BAKED_LANES_MASK)) return KNERF_ERR_INVALID;
    if ((flags & KNERF_BAKED_SKIP_EMPTY) && !field->bits) return KNERF_ERR_INVALID;
    if (!(step > 0.f) || !std::isfinite(step) || !(termination >= 0.f) || !(termination < 1.f)) return KNERF_ERR_INVALID;
    if ((!near && !std::isfinite(near_all)) || (!far && !std::isfinite(far_all))) return KNERF_ERR_INVALID;
    const int L = field->brick_log2;
    if (L != 2 && L != 3) return KNERF_ERR_INVALID;
    bricks::RenderArgs a{};
    unsigned long long points = 1, grid = 1;
    int B[3];
    for (int c = 0; c < 3; ++c) {
        const int r = field->resolution[c];
        if (r < 2 || r > 1025) return KNERF_ERR_INVALID;
        if (!std::isfinite(field->lo[c]) || !std::isfinite(field->hi[c]) || !(field->hi[c] > field->lo[c])) return KNERF_ERR_INVALID;
        a.R[c] = r; a.lo[c] = field->lo[c]; a.hi[c] = field->hi[c];
        a.scale[c] = (float)((double)(r - 1) / ((double)field->hi[c] - (double)field->lo[c]));
        if (!std::isfinite(a.scale[c])) return KNERF_ERR_INVALID;
        points *= (unsigned)r;
        B[c] = (r + (1 << L) - 1) >> L;
        grid *= (unsigned)B[c];
    }
    // what knerf_baked_render refuses for the same lattice is refused here as well, although the dense table is never formed
    if (points >= bricks::kMaxBytes / (unsigned)bricks::rec_bytes(deg)) return KNERF_ERR_INVALID;
    if (field->n_bricks == 0 || field->n_bricks > grid) return KNERF_ERR_INVALID;
    if ((field->n_bricks << (3 * L)) >= bricks::kMaxBytes / (unsigned)bricks::rec_bytes(deg)) return KNERF_ERR_INVALID;
    int lanes = (flags & KNERF_BAKED_LANES_MASK) >> KNERF_BAKED_LANES_SHIFT;
    if (lanes == 0) lanes = deg == 0 ? 1 : (deg == 1 ? 2 : 4);
    if (!(lanes == 1 || (lanes == 2 && deg == 1) || (lanes == 4 && deg >= 2))) return KNERF_ERR_INVALID;
    if (n_rays >= (1ull << 36)) return KNERF_ERR_INVALID;
    if (n_rays == 0) return KNERF_OK;
    a.rec = static_cast<const uint4*>(field->records); a.brick_of = field->brick_of; a.bits = field->bits;
    a.L = L; a.By = B[1]; a.Bz = B[2]; a.n_bricks = (long long)field->n_bricks;
    a.o = origins; a.d = directions; a.near = near; a.far = far; a.near0 = near_all; a.far0 = far_all;
    a.n = (long long)n_rays; a.step = step; a.eps = termination;
    a.white = (flags & KNERF_BAKED_WHITE_BACKGROUND) ? 1 : 0; a.skip = (flags & KNERF_BAKED_SKIP_EMPTY) ? 1 : 0;
    a.image = image; a.depth = depth; a.opacity = opacity; a.stats = reinterpret_cast<unsigned long long*>(stats);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipErrorInvalidValue;
    switch (deg * 8 + lanes) {
        case 0 * 8 + 1: e = bricks::launch_render<0, 1>(a, s); break;
        case 1 * 8 + 1: e = bricks::launch_render<1, 1>(a, s); break;
        case 1 * 8 + 2: e = bricks::launch_render<1, 2>(a, s); break;
        case 2 * 8 + 1: e = bricks::launch_render<2, 1>(a, s); break;
        case 2 * 8 + 4: e = bricks::launch_render<2, 4>(a, s); break;
        case 3 * 8 + 1: e = bricks::launch_render<3, 1>(a, s); break;
        case 3 * 8 + 4: e = bricks::launch_render<3, 4>(a, s); break;
        default: return KNERF_ERR_INVALID;
    }
    return e == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
