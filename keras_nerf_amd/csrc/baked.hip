// baked.hip -- the trained field baked into a voxel grid with spherical-harmonic colour, and its renderer for dense and for brick
// storage (gfx950), context-free.  Extension: the reference has nothing of the kind (PlenOctrees / SNeRG / Plenoxels bake a trained NeRF
// in this way, and store only the occupied part of their grids behind a coarse index).  What the file shares with the other
// baked*.hip files is in baked_common.h.
//
// Lattice [Rx][Ry][Rz] (C order, z fastest) placed as in knerf_query_grid.  One RECORD per lattice point (include/knerf.h):
//   bytes 0..3   fp32 sigma (after ReLU; values <= the bake's threshold are stored as 0)
//   then 3 K halfs, K = (degree + 1)^2, ordered [k][c]: coefficient k of channel c at half slot 2 + 3 k + c
//   zero padding to a multiple of 16 bytes: 16 / 32 / 64 / 112 bytes for degree 0 / 1 / 2 / 3
// A record is read in 16-byte CHUNKS (8 half slots each); chunk 0 starts with sigma.
//
// Brick storage: the lattice is cut into BRICKS of b^3 lattice points, b = 1 << brick_log2 = 4 or 8: point (x, y, z) lies in brick
// (x >> L, y >> L, z >> L) of the brick grid B_a = ceil(R_a / b), at place ((x & (b-1)) b + (y & (b-1))) b + (z & (b-1)) in it.
//   brick_of  int32 [Bx][By][Bz]: the slot of a stored brick, -1 for an absent one
//   records   [n_bricks][b^3] records in the layout above
// A point of an absent brick reads as an all-zero record.  A brick_of value outside [0, n_bricks) counts as absent: a damaged table
// never becomes an out-of-range read.  The occupancy bits are those of the dense field.
//
//   baked_project_kernel   acc[n][k][c] += P[k][j] rgb[n][c]: one direction of the least-squares SH fit; one fused multiply-add, or with
//                          a second buffer a compensated sum (the rounding errors of product and sum, both exact, are kept beside it)
//   baked_pack_kernel      acc (+ comp) -> fp16 (round to nearest even), sigma and coefficients scattered into the records
//   baked_render_kernel    <DEG, G, Args>: G lanes march one ray; lane `sub` of the group owns chunks sub, sub + G, ... of every record it
//                          meets.  G = 1 is one ray per lane (8 corners x record bytes per lane and sample); with G = record chunks
//                          the group reads each corner as ONE contiguous record.  Every lane of a group runs the whole march on the
//                          same numbers (same control flow); the three channel sums are added across the group with DPP quad
//                          permutes and sigma comes from the lane that owns chunk 0.  One ray's samples are never split across lanes:
//                          compositing is strictly in ascending sample order, so skipping empty cells is exact (see below).
//                          Args = RenderArgs (dense) or BrickRenderArgs: ONE march for both storages, so every sample's arithmetic
//                          is the same and the outputs are bit-identical (tests/test_gpu_baked_bricks.py holds the two in step).
//                          Only the record address differs (Args::kBrick): the dense address is plain arithmetic formed at its load;
//                          the 8 brick addresses are formed through brick_of in front of the record loads, so the
//                          loads still issue together (the march is bound by memory latency).  With b = 8 about two thirds of the
//                          samples have all 8 corners in the brick the lane looked up last, so most samples need no table read.
//
// The march of one ray (include/knerf.h knerf_baked_render restates it; tests/baked_reference.py is the fp64 restatement):
//   S = ceil((far - near) / step) in double; t_i = near + (i + 0.5) step; p = __fadd_rn(o, __fmul_rn(d, t_i)).
//   The slab intersection only narrows [i0, i1) (two samples of margin each side); whether a sample is inside is decided per sample
//   from u = (p - lo) * scale: inside iff 0 <= u <= cells on every axis; cell = min(floor(u), cells - 1), weights from u - cell.
//   alpha = 1 - expf(-(sigma * (step |d|))), w = T alpha, image += w colour, depth += w t_i, opacity += w, T <- T (1 - alpha).
//   The samples are visited in batches of kBatch: first the occupancy words of the batch are loaded together (the march is bound by
//   memory latency, and a dependent bit load per sample cost more than it saved), then the samples to fetch are composited in order.
//   An empty cell has sigma = 0 at all 8 corners: trilinear sigma = 0 exactly, alpha = 0, w = 0, T unchanged; not fetching the sample
//   gives the same bits.
#include "baked_common.h"

namespace knerf {
namespace baked {

// ---- bake: projection onto the SH basis and packing
__global__ void baked_project_kernel(const float* __restrict__ rgb, const float* __restrict__ fit, int K, int D, int j, long long n,
                                     float* __restrict__ acc, float* __restrict__ comp) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int E = 3 * K;
    if (idx >= n * E) return;
    const long long p = idx / E;
    const int e = (int)(idx - p * E), k = e / 3, c = e - 3 * k;
    const float w = fit[(long long)k * D + j], x = rgb[p * 3 + c], a = acc[idx];
    if (!comp) { acc[idx] = __builtin_fmaf(w, x, a); return; }
    // compensated: the product's and the sum's rounding errors (both exact in fp32) are collected in comp
    const float prod = __fmul_rn(w, x), perr = __builtin_fmaf(w, x, -prod);
    const float s = __fadd_rn(a, prod), bb = __fsub_rn(s, a);
    const float serr = __fadd_rn(__fsub_rn(a, __fsub_rn(s, bb)), __fsub_rn(prod, bb));
    acc[idx] = s;
    comp[idx] = __fadd_rn(comp[idx], __fadd_rn(serr, perr));
}

__global__ void baked_pack_kernel(const float* __restrict__ sigma, const float* __restrict__ acc, const float* __restrict__ comp,
                                  const long long* __restrict__ index, long long n, long long n_points, int K, int nch, uint4* __restrict__ rec) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * nch) return;
    const long long i = idx / nch;
    const int q = (int)(idx - i * nch);
    const long long p = index ? index[i] : i;
    if (p < 0 || p >= n_points) return;
    unsigned h[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int e = 8 * q - 2 + s;
        const bool on = e >= 0 && e < 3 * K;
        const long long at = i * (3 * K) + (on ? e : 0);
        h[s] = on ? float_to_half_bits(comp ? __fadd_rn(acc[at], comp[at]) : acc[at]) : 0u;
    }
    uint4 v;
    v.x = q == 0 ? __float_as_uint(sigma[p]) : (h[0] | (h[1] << 16));
    v.y = h[2] | (h[3] << 16);
    v.z = h[4] | (h[5] << 16);
    v.w = h[6] | (h[7] << 16);
    rec[p * nch + q] = v;
}

// ---- render
struct RenderArgs {
    static constexpr bool kBrick = false;
    const uint4* rec;
    const unsigned* bits;
    int R[3];
    float lo[3], hi[3], scale[3];
    const float *o, *d, *near, *far;
    float near0, far0;
    long long n;
    float step, eps;
    int white, skip;
    float *image, *depth, *opacity;
    unsigned long long* stats;
};

struct BrickRenderArgs {
    static constexpr bool kBrick = true;
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

template <int DEG, int G, class Args>
__global__ __launch_bounds__(kBlock) void baked_render_kernel(Args a) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, CPL = (NCH + G - 1) / G;     // chunks per record / per lane
    constexpr bool BRICK = Args::kBrick;
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
        [[maybe_unused]] const long long sy = a.R[2], sx = (long long)a.R[1] * a.R[2];     // dense: the lattice's strides
        const int cyc = a.R[1] - 1, czc = a.R[2] - 1;
        [[maybe_unused]] const int L = brick_log2(a), inm = (1 << L) - 1;
        // BRICK: the brick this lane looked up last (linear brick index and slot): consecutive samples mostly stay in one brick.  (One
        // entry per corner was measured too: 26 more VGPRs, a wave per SIMD fewer, 9 % slower.)
        [[maybe_unused]] int last_key = -1, last_slot = -1;
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
            // The dense address is plain arithmetic and is formed at its load: put in front as well it cost time (measured in the
            // ray-gradient kernels, 3.8 against 3.0 ms).  BRICK: the 8 corner records through the brick table, in front of the loads, so
            // that the loads still issue together: at[cn] < 0 = a point of an absent brick
            [[maybe_unused]] const long long base = (long long)ci[0] * sx + (long long)ci[1] * sy + ci[2];
            [[maybe_unused]] int at[8];
            if constexpr (BRICK) {
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
#pragma unroll
                for (int cn = 0; cn < 8; ++cn) {
                    const int x = ci[0] + ((cn >> 2) & 1), y = ci[1] + ((cn >> 1) & 1), z = ci[2] + (cn & 1);
                    const int in = ((((x & inm) << L) | (y & inm)) << L) | (z & inm);
                    const bool stored = slot[cn] >= 0 && (long long)slot[cn] < a.n_bricks;
                    at[cn] = stored ? (int)(((unsigned)slot[cn] << (3 * L)) + (unsigned)in) : -1;
                }
            }
            float sig = 0.f, cf[CPL][8];
#pragma unroll
            for (int j = 0; j < CPL; ++j)
#pragma unroll
                for (int s = 0; s < 8; ++s) cf[j][s] = 0.f;
#pragma unroll
            for (int cn = 0; cn < 8; ++cn) {
                const float w = ((cn & 4) ? fr[0] : 1.f - fr[0]) * ((cn & 2) ? fr[1] : 1.f - fr[1]) * ((cn & 1) ? fr[2] : 1.f - fr[2]);
                long long pt;
                if constexpr (BRICK) pt = at[cn];                   // (sign-extended: -1 stays -1)
                else pt = base + ((cn & 4) ? sx : 0) + ((cn & 2) ? sy : 0) + (cn & 1);
                uint4 v[CPL];
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const int qc = sub + j * G;
                    v[j] = (qc < NCH && (!BRICK || pt >= 0)) ? a.rec[pt * NCH + qc] : make_uint4(0u, 0u, 0u, 0u);
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

template <class Args>
hipError_t launch_render(int deg, int lanes, const Args& a, hipStream_t s) {
    return dispatch_deg_lanes(deg, lanes, [&](auto DEG, auto G) {
        const long long blocks = (a.n * G + kBlock - 1) / kBlock;
        hipLaunchKernelGGL((baked_render_kernel<DEG, G, Args>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
        return hipGetLastError();
    });
}

// what both renderers check of their arguments beside the field; lanes comes back resolved.  n_rays = 0 is for the caller
static bool check_render(int deg, const unsigned* bits, const float* origins, const float* directions, const float* near,
                         const float* far, float near_all, float far_all, uint64_t n_rays, float step, float termination, int flags,
                         const float* image, const float* depth, const float* opacity, const int64_t* stats, int& lanes) {
    if (!origins || !directions) return false;
    if (!image && !depth && !opacity && !stats) return false;
    if (!check_rays(near, far, near_all, far_all, n_rays, step, termination, flags)) return false;
    if ((flags & KNERF_BAKED_SKIP_EMPTY) && !bits) return false;
    lanes = pick_lanes(deg, flags, kLaneGroups);
    return lanes != 0;
}

// the ray arguments and outputs, the same fields in both argument structs
template <class Args>
static void set_rays(Args& a, const float* origins, const float* directions, const float* near, const float* far, float near_all,
                     float far_all, uint64_t n_rays, float step, float termination, int flags, float* image, float* depth,
                     float* opacity, int64_t* stats) {
    a.o = origins; a.d = directions; a.near = near; a.far = far; a.near0 = near_all; a.far0 = far_all;
    a.n = (long long)n_rays; a.step = step; a.eps = termination;
    a.white = (flags & KNERF_BAKED_WHITE_BACKGROUND) ? 1 : 0; a.skip = (flags & KNERF_BAKED_SKIP_EMPTY) ? 1 : 0;
    a.image = image; a.depth = depth; a.opacity = opacity; a.stats = reinterpret_cast<unsigned long long*>(stats);
}

}  // namespace baked
}  // namespace knerf

using namespace knerf;

extern "C" int knerf_baked_project(void* stream, const float* rgb, const float* fit, int n_coeff, int n_dirs, int j, uint64_t n, float* acc,
                                   float* comp) {
    if (!rgb || !fit || !acc || n_dirs < 1 || j < 0 || j >= n_dirs) return KNERF_ERR_INVALID;
    if (n_coeff != 1 && n_coeff != 4 && n_coeff != 9 && n_coeff != 16) return KNERF_ERR_INVALID;
    if (n >= (1ull << 40) / (12ull * (unsigned)n_coeff)) return KNERF_ERR_INVALID;
    if (n == 0) return KNERF_OK;
    const unsigned long long elems = n * 3ull * (unsigned)n_coeff, blocks = (elems + 255) / 256;
    if (blocks >= (1ull << 31)) return KNERF_ERR_INVALID;
    hipLaunchKernelGGL(baked::baked_project_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rgb, fit, n_coeff, n_dirs, j,
                       (long long)n, acc, comp);
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_pack(void* stream, const float* sigma, const float* acc, const float* comp, const int64_t* index, uint64_t n,
                                uint64_t n_points, int sh_degree, void* records) {
    if (!sigma || !acc || !records || sh_degree < 0 || sh_degree > 3 || n_points == 0 || n > n_points) return KNERF_ERR_INVALID;
    if (!index && n != n_points) return KNERF_ERR_INVALID;
    const unsigned rec = (unsigned)baked::rec_bytes(sh_degree);
    if (n_points >= baked::kMaxBytes / rec) return KNERF_ERR_INVALID;
    if (n == 0) return KNERF_OK;
    const int nch = (int)rec / 16;
    const unsigned long long blocks = (n * (unsigned)nch + 255) / 256;
    if (blocks >= (1ull << 31)) return KNERF_ERR_INVALID;
    hipLaunchKernelGGL(baked::baked_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, sigma, acc, comp,
                       reinterpret_cast<const long long*>(index), (long long)n, (long long)n_points, baked::n_coeff(sh_degree), nch,
                       static_cast<uint4*>(records));
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_render(void* stream, const knerf_baked_field* field, const float* origins, const float* directions,
                                  const float* near, const float* far, float near_all, float far_all, uint64_t n_rays, float step,
                                  float termination, int flags, float* image, float* depth, float* opacity, int64_t* stats) {
    if (!field || !field->records) return KNERF_ERR_INVALID;
    baked::RenderArgs a{};
    unsigned long long points = 0;
    int lanes = 0;
    const int deg = field->sh_degree;
    if (!baked::check_lattice(field->resolution, field->lo, field->hi, deg, a.scale, points)) return KNERF_ERR_INVALID;
    if (!baked::check_render(deg, field->bits, origins, directions, near, far, near_all, far_all, n_rays, step, termination, flags, image,
                             depth, opacity, stats, lanes))
        return KNERF_ERR_INVALID;
    if (n_rays == 0) return KNERF_OK;
    for (int c = 0; c < 3; ++c) { a.R[c] = field->resolution[c]; a.lo[c] = field->lo[c]; a.hi[c] = field->hi[c]; }
    a.rec = static_cast<const uint4*>(field->records); a.bits = field->bits;
    baked::set_rays(a, origins, directions, near, far, near_all, far_all, n_rays, step, termination, flags, image, depth, opacity, stats);
    return baked::launch_render(deg, lanes, a, (hipStream_t)stream) == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_render_bricks(void* stream, const knerf_baked_bricks* field, const float* origins, const float* directions,
                                         const float* near, const float* far, float near_all, float far_all, uint64_t n_rays, float step,
                                         float termination, int flags, float* image, float* depth, float* opacity, int64_t* stats) {
    if (!field || !field->records || !field->brick_of) return KNERF_ERR_INVALID;
    baked::BrickRenderArgs a{};
    unsigned long long points = 0;
    int lanes = 0, B[3];
    const int deg = field->sh_degree;
    // what knerf_baked_render refuses for the same lattice is refused here as well, although the dense table is never formed
    if (!baked::check_lattice(field->resolution, field->lo, field->hi, deg, a.scale, points)) return KNERF_ERR_INVALID;
    if (!baked::check_brick_grid(field->resolution, deg, field->brick_log2, field->n_bricks, B)) return KNERF_ERR_INVALID;
    if (!baked::check_render(deg, field->bits, origins, directions, near, far, near_all, far_all, n_rays, step, termination, flags, image,
                             depth, opacity, stats, lanes))
        return KNERF_ERR_INVALID;
    if (n_rays == 0) return KNERF_OK;
    for (int c = 0; c < 3; ++c) { a.R[c] = field->resolution[c]; a.lo[c] = field->lo[c]; a.hi[c] = field->hi[c]; }
    a.rec = static_cast<const uint4*>(field->records); a.brick_of = field->brick_of; a.bits = field->bits;
    a.L = field->brick_log2; a.By = B[1]; a.Bz = B[2]; a.n_bricks = (long long)field->n_bricks;
    baked::set_rays(a, origins, directions, near, far, near_all, far_all, n_rays, step, termination, flags, image, depth, opacity, stats);
    return baked::launch_render(deg, lanes, a, (hipStream_t)stream) == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
