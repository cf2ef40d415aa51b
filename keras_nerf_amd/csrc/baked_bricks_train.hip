// baked_bricks_train.hip -- optimising a baked field that is stored as sparse bricks (gfx950), context-free: the gradient launch and the
// Adam launch of baked_train.hip on the brick layout of baked_bricks.hip, so that the dense record table is never formed.  Extension: the
// reference has nothing of the kind.  include/knerf.h holds the contract.  Neither baked_train.hip nor baked_bricks.hip is touched: the
// march, its helpers and the Adam arithmetic are restated here (same constants, same operations, same order), and
// tests/test_gpu_baked_bricks_train.py holds the restatement in step with the dense kernels bit for bit.
//
//   baked_bricks_train_rays_kernel   <DEG, G>: baked_train_rays_kernel word for word -- both marches, the total-minus-prefix suffix sum,
//                             the dsig / dr zero test, the trilinear weights, the column-per-lane atomic scatter, sq_err.  Only a
//                             corner's address differs: it is formed through brick_of as in baked_render_bricks_kernel, with the lane's
//                             one-entry cache of the brick it looked up last; an entry < 0 or >= n_bricks counts as absent BEFORE any
//                             address is formed, an absent corner's record reads as zero and NOTHING is added for it, so a damaged table
//                             never becomes an out-of-range read or write.  There is no slot table: the rows of gradient, master value and
//                             moments are per STORED RECORD, and a row's index is the record's index.
//   baked_bricks_train_apply_kernel  one lane per (record, chunk): the arithmetic of baked_train_apply_kernel.  flags[record] bit 0: the
//                             record is a slot (a corner of a support cell); a record without it is skipped entirely.  Bit 1: sigma is
//                             trainable there.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/knerf.h"

namespace knerf {
namespace bricks_train {

constexpr int kBlock = 256;
constexpr int kBatch = 8;                           // as baked.hip: samples whose support bits are looked up together
constexpr int kMaxSamples = 1 << 23;
constexpr unsigned long long kMaxBytes = 1ull << 40;

__host__ __device__ constexpr int n_coeff(int deg) { return (deg + 1) * (deg + 1); }
__host__ __device__ constexpr int rec_bytes(int deg) { return (4 + 6 * n_coeff(deg) + 15) / 16 * 16; }

__device__ __forceinline__ float half_bits_to_float(unsigned h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(h & 0xffffu)); }
__device__ __forceinline__ unsigned float_to_half_bits(float f) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)f); }   // round to nearest even

struct TrainArgs {
    const uint4* rec;
    const int* brick_of;
    const unsigned* bits;
    int R[3];
    int L, By, Bz;                                  // log2 of the brick edge; the brick grid's y and z extents
    long long n_bricks;
    float lo[3], hi[3], scale[3];
    const float *o, *d, *near, *far, *target;
    float near0, far0;
    long long n;
    float step, eps, gscale;                        // gscale = 2 / (3 N)
    int white;
    float* grad;
    float* sq_err;
};

// the basis of baked.hip sh_eval
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

__device__ __forceinline__ bool locate(const TrainArgs& a, float near, const float (&o3)[3], const float (&d3)[3], int i, float& t,
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

// what the second march needs from the first: g = dL/dout (already gated by the output clamp) and the totals
struct Totals {
    float g[3], img[3], opa, bg;
};

// One march of one ray over the samples [i, i1), as march of baked_train.hip.  BWD = false: img / opa end as C / O.  BWD = true: the same
// arithmetic again (img / opa are then the prefix sums), and per sample the gradient is added.
template <int DEG, int G, bool BWD>
__device__ __forceinline__ void march(const TrainArgs& a, const float (&o3)[3], const float (&d3)[3], float near, int i, int i1,
                                      float delta, int sub, const float (&Y)[n_coeff(DEG)],
                                      const float (&wr)[(rec_bytes(DEG) / 16 + G - 1) / G][8],
                                      const float (&wg)[(rec_bytes(DEG) / 16 + G - 1) / G][8],
                                      const float (&wb)[(rec_bytes(DEG) / 16 + G - 1) / G][8],
                                      const float (&gy)[(1 + 3 * n_coeff(DEG) + G - 1) / G][3], float (&img)[3], float& opa, const Totals& tt) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, CPL = (NCH + G - 1) / G, W = 1 + 3 * K, NI = (W + G - 1) / G;
    const int cyc = a.R[1] - 1, czc = a.R[2] - 1;
    const int L = a.L, inm = (1 << L) - 1;
    int last_key = -1, last_slot = -1;                  // the brick this lane looked up last, as baked_bricks.hip
    float T = 1.f;
    img[0] = img[1] = img[2] = 0.f;
    opa = 0.f;
    bool done = false;
    for (; i < i1 && !done; i += kBatch) {
        unsigned mask = 0;
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            int cj[3];
            float fj[3], tj;
            const bool need = i + k < i1 && locate(a, near, o3, d3, i + k, tj, cj, fj);
            const unsigned b = need ? ((unsigned)cj[0] * (unsigned)cyc + (unsigned)cj[1]) * (unsigned)czc + (unsigned)cj[2] : 0u;
            const unsigned word = a.bits[b >> 5];
            if (need && ((word >> (b & 31u)) & 1u)) mask |= 1u << k;
        }
        while (mask) {
            const int kk = __builtin_ctz(mask);
            mask &= mask - 1u;
            int ci[3];
            float fr[3], t;
            locate(a, near, o3, d3, i + kk, t, ci, fr);
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
            // a record's index fits 32 bits (n_bricks <= Bx By Bz, so at most 1032^3 records); byte offsets are formed in 64
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
                    const bool first = j == 0 && sub == 0;
                    if (j == 0) sig = __builtin_fmaf(w, first ? __uint_as_float(wd[0]) : 0.f, sig);
#pragma unroll
                    for (int s = 0; s < 8; ++s) {
                        cf[j][s] = __builtin_fmaf(w, half_bits_to_float(wd[s >> 1] >> ((s & 1) * 16)), cf[j][s]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int e = 8 * (sub + j * G) - 2 + s;
                    cf[j][s] = (e >= 0 && e < 3 * K) ? cf[j][s] : 0.f;
                }
            }
            float raw[3] = {0.f, 0.f, 0.f};
            if constexpr (G == 1) {
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
#pragma unroll
                    for (int s = 0; s < 8; ++s) {
                        const int e = 8 * j - 2 + s;
                        if (e >= 0 && e < 3 * K) raw[e % 3] = __builtin_fmaf(cf[j][s], Y[e / 3], raw[e % 3]);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
#pragma unroll
                    for (int s = 0; s < 8; ++s) {
                        raw[0] = __builtin_fmaf(cf[j][s], wr[j][s], raw[0]);
                        raw[1] = __builtin_fmaf(cf[j][s], wg[j][s], raw[1]);
                        raw[2] = __builtin_fmaf(cf[j][s], wb[j][s], raw[2]);
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) raw[c] = group_sum<G>(raw[c]);
                sig = group_first<G>(sig);
            }
            float col[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) col[c] = fminf(fmaxf(raw[c], 0.f), 1.f);
            const float alpha = 1.f - expf(-(sig * delta));
            const float w = T * alpha;
            img[0] = img[0] + w * col[0]; img[1] = img[1] + w * col[1]; img[2] = img[2] + w * col[2];
            opa = opa + w;
            T = T * (1.f - alpha);
            if constexpr (BWD) {
                // A_j = sum_c g_c (col_jc - bg); the later samples' share is total minus prefix (the prefix includes sample j)
                float A = 0.f, later = 0.f, dr[3];
                const float rest_o = tt.opa - opa;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    A = __builtin_fmaf(tt.g[c], col[c] - tt.bg, A);
                    later = __builtin_fmaf(tt.g[c], (tt.img[c] - img[c]) - tt.bg * rest_o, later);
                    dr[c] = (raw[c] >= 0.f && raw[c] <= 1.f) ? tt.g[c] * w : 0.f;
                }
                const float dsig = delta * (T * A - later);           // T is T_{j+1} here
                if (dsig != 0.f || dr[0] != 0.f || dr[1] != 0.f || dr[2] != 0.f) {     // the same on every lane of the group
#pragma unroll
                    for (int cn = 0; cn < 8; ++cn) {
                        const float tw = ((cn & 4) ? fr[0] : 1.f - fr[0]) * ((cn & 2) ? fr[1] : 1.f - fr[1]) * ((cn & 1) ? fr[2] : 1.f - fr[2]);
                        const long long pt = at[cn];
                        if (pt < 0) continue;                            // a point of an absent brick has no row: nothing is added
                        float* row = a.grad + pt * W;
                        // lane `sub` adds the columns sub, sub + G, ...: one instruction of the group adds G consecutive floats of the row
#pragma unroll
                        for (int s = 0; s < NI; ++s) {
                            const int col = s * G + sub;
                            float val;
                            if constexpr (G == 1) {
                                val = s == 0 ? dsig : Y[(s > 0 ? s - 1 : 0) / 3] * dr[(s > 0 ? s - 1 : 0) % 3];
                            } else {
                                val = __builtin_fmaf(gy[s][0], dr[0], __builtin_fmaf(gy[s][1], dr[1], gy[s][2] * dr[2]));
                                val = col == 0 ? dsig : val;
                            }
                            if (col < W) atomicAdd(row + col, tw * val);
                        }
                    }
                }
            }
            if (a.eps > 0.f && T < a.eps) { done = true; break; }
        }
    }
}

template <int DEG, int G>
__global__ __launch_bounds__(kBlock) void baked_bricks_train_rays_kernel(TrainArgs a) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, CPL = (NCH + G - 1) / G;
    static_assert(G == 1 || G == 2 || G == 4, "a group is a lane, a pair or a quad");
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long ray = gid / G;
    const int sub = (int)(gid & (G - 1));
    if (ray >= a.n) return;
    const float ox = a.o[ray * 3 + 0], oy = a.o[ray * 3 + 1], oz = a.o[ray * 3 + 2];
    const float dx = a.d[ray * 3 + 0], dy = a.d[ray * 3 + 1], dz = a.d[ray * 3 + 2];
    const float near = a.near ? a.near[ray] : a.near0, far = a.far ? a.far[ray] : a.far0;
    const float nrm = __fsqrt_rn(dx * dx + dy * dy + dz * dz);
    const float ux = nrm > 0.f ? dx / nrm : 0.f, uy = nrm > 0.f ? dy / nrm : 0.f, uz = nrm > 0.f ? dz / nrm : 0.f;
    float Y[K];
    sh_eval<DEG>(ux, uy, uz, Y);
    float wr[CPL][8], wg[CPL][8], wb[CPL][8];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int e = 8 * (sub + j * G) - 2 + s;
            const int k = e / 3, c = e - 3 * k;
            float yk = 0.f;
            if constexpr (G > 1) {
#pragma unroll
                for (int kk = 0; kk < K; ++kk) yk = (e >= 0 && k == kk) ? Y[kk] : yk;
            }
            wr[j][s] = c == 0 ? yk : 0.f; wg[j][s] = c == 1 ? yk : 0.f; wb[j][s] = c == 2 ? yk : 0.f;
        }
    }
    // G > 1: the basis value and channel of the gradient columns this lane adds, columns sub, sub + G, ... of a row (column 0 is sigma)
    constexpr int NI = (1 + 3 * K + G - 1) / G;
    float gy[NI][3];
#pragma unroll
    for (int s = 0; s < NI; ++s) {
        const int e = s * G + sub - 1;
        const int k = e / 3, c = e - 3 * k;
        float yk = 0.f;
        if constexpr (G > 1) {
#pragma unroll
            for (int kk = 0; kk < K; ++kk) yk = (e >= 0 && k == kk) ? Y[kk] : yk;
        }
        gy[s][0] = c == 0 ? yk : 0.f; gy[s][1] = c == 1 ? yk : 0.f; gy[s][2] = c == 2 ? yk : 0.f;
    }
    const double q = ((double)far - (double)near) / (double)a.step;
    const int S = q > 0.0 ? (q >= (double)kMaxSamples ? kMaxSamples : (int)ceil(q)) : 0;
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
    int i0 = 0, i1 = 0;
    if (!miss && S > 0) {
        const double a0 = floor(((double)tmin - (double)near) / (double)a.step - 0.5) - 2.0;
        const double a1 = floor(((double)tmax - (double)near) / (double)a.step - 0.5) + 3.0;
        i0 = (int)fmin(fmax(a0, 0.0), (double)S);
        i1 = (int)fmin(fmax(a1, 0.0), (double)S);
    }
    const float delta = a.step * nrm;
    Totals tt{};
    march<DEG, G, false>(a, o3, d3, near, i0, i1, delta, sub, Y, wr, wg, wb, gy, tt.img, tt.opa, tt);
    tt.bg = a.white ? 1.f : 0.f;
    const float bg = a.white ? 1.f - tt.opa : 0.f;          // the render kernel's expression
    float sq = 0.f;
    bool any = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float pre = tt.img[c] + bg, out = fminf(fmaxf(pre, 0.f), 1.f);
        const float diff = out - a.target[ray * 3 + c];
        sq = sq + diff * diff;
        tt.g[c] = (pre >= 0.f && pre <= 1.f) ? diff * a.gscale : 0.f;
        any = any || tt.g[c] != 0.f;
    }
    if (sub == 0 && a.sq_err) a.sq_err[ray] = sq;
    if (!any) return;                                       // the same on every lane of the group
    float img[3], opa;
    march<DEG, G, true>(a, o3, d3, near, i0, i1, delta, sub, Y, wr, wg, wb, gy, img, opa, tt);
}

template <int DEG, int G>
hipError_t launch_rays(const TrainArgs& a, hipStream_t s) {
    const long long lanes = a.n * G, blocks = (lanes + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((baked_bricks_train_rays_kernel<DEG, G>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

struct ApplyArgs {
    uint4* rec;
    const unsigned char* flags;
    float *w, *m, *v, *g;
    long long n_records;
    int K, nch;
    float rate_sigma, rate_sh, b1, b2, eps;
};

__device__ __forceinline__ float adam(const ApplyArgs& a, long long at, float rate, bool train) {
    const float g = a.g[at];
    a.g[at] = 0.f;
    float w = a.w[at];
    if (!train) return w;
    float m = a.m[at], v = a.v[at];
    m = m + (g - m) * (1.f - a.b1);
    v = v + (g * g - v) * (1.f - a.b2);
    a.m[at] = m; a.v[at] = v;
    return w - rate * m / (sqrtf(v) + a.eps);
}

__global__ __launch_bounds__(256) void baked_bricks_train_apply_kernel(ApplyArgs a) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n_records * a.nch) return;
    const long long record = idx / a.nch;
    const int q = (int)(idx - record * a.nch);
    const unsigned flag = a.flags[record];
    if (!(flag & 1u)) return;                                   // not a slot: record, master, moments and gradient keep their bytes
    const long long row = record * (1 + 3 * a.K);
    float sig = 0.f;
    if (q == 0) {
        sig = fmaxf(adam(a, row, a.rate_sigma, (flag & 2u) != 0), 0.f);           // the projection; an untrainable sigma is and stays 0
        a.w[row] = sig;
    }
    unsigned h[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int e = 8 * q - 2 + s;
        h[s] = 0u;
        if (e >= 0 && e < 3 * a.K) {
            const float w = adam(a, row + 1 + e, a.rate_sh, true);
            a.w[row + 1 + e] = w;
            h[s] = float_to_half_bits(w);
        }
    }
    uint4 out;
    out.x = q == 0 ? __float_as_uint(sig) : (h[0] | (h[1] << 16));
    out.y = h[2] | (h[3] << 16);
    out.z = h[4] | (h[5] << 16);
    out.w = h[6] | (h[7] << 16);
    a.rec[record * a.nch + q] = out;
}

// the checks both entry points share: what knerf_baked_render_bricks refuses of its struct, and the NULLs this one adds
static bool check_state(const knerf_baked_bricks_train* t, int (&B)[3], double (&scale)[3], unsigned long long& n_records) {
    if (!t || !t->field.records || !t->field.brick_of || !t->field.bits || !t->grad) return false;
    const knerf_baked_bricks* f = &t->field;
    const int deg = f->sh_degree;
    if (deg < 0 || deg > 3) return false;
    const int L = f->brick_log2;
    if (L != 2 && L != 3) return false;
    unsigned long long points = 1, grid = 1;
    for (int c = 0; c < 3; ++c) {
        const int r = f->resolution[c];
        if (r < 2 || r > 1025) return false;
        if (!std::isfinite(f->lo[c]) || !std::isfinite(f->hi[c]) || !(f->hi[c] > f->lo[c])) return false;
        scale[c] = (double)(r - 1) / ((double)f->hi[c] - (double)f->lo[c]);
        if (!std::isfinite((float)scale[c])) return false;
        points *= (unsigned)r;
        B[c] = (r + (1 << L) - 1) >> L;
        grid *= (unsigned)B[c];
    }
    if (points >= kMaxBytes / (unsigned)rec_bytes(deg)) return false;
    if (f->n_bricks == 0 || f->n_bricks > grid) return false;
    if ((f->n_bricks << (3 * L)) >= kMaxBytes / (unsigned)rec_bytes(deg)) return false;
    n_records = f->n_bricks << (3 * L);
    return true;
}

}  // namespace bricks_train
}  // namespace knerf

using namespace knerf;

extern "C" int knerf_baked_bricks_train_rays(void* stream, const knerf_baked_bricks_train* train, const float* origins,
                                             const float* directions, const float* near, const float* far, float near_all, float far_all,
                                             const float* target, uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags,
                                             float* sq_err) {
    int B[3];
    double scale[3];
    unsigned long long n_records = 0;
    if (!bricks_train::check_state(train, B, scale, n_records) || !origins || !directions || !target) return KNERF_ERR_INVALID;
    if (flags & ~(KNERF_BAKED_WHITE_BACKGROUND | KNERF_BAKED_SKIP_EMPTY | KNERF_BAKED_LANES_MASK)) return KNERF_ERR_INVALID;
    if (!(step > 0.f) || !std::isfinite(step) || !(termination >= 0.f) || !(termination < 1.f)) return KNERF_ERR_INVALID;
    if ((!near && !std::isfinite(near_all)) || (!far && !std::isfinite(far_all))) return KNERF_ERR_INVALID;
    const knerf_baked_bricks* field = &train->field;
    const int deg = field->sh_degree;
    bricks_train::TrainArgs a{};
    for (int c = 0; c < 3; ++c) {
        a.R[c] = field->resolution[c]; a.lo[c] = field->lo[c]; a.hi[c] = field->hi[c];
        a.scale[c] = (float)scale[c];
    }
    // every lane variant of knerf_baked_train_rays exists here too: each builds without scratch (DESIGN.md 2.23 has hipcc's counts)
    int lanes = (flags & KNERF_BAKED_LANES_MASK) >> KNERF_BAKED_LANES_SHIFT;
    if (lanes == 0) lanes = deg == 0 ? 1 : (deg == 1 ? 2 : 4);
    if (!(lanes == 1 || (lanes == 2 && deg == 1) || (lanes == 4 && deg >= 2))) return KNERF_ERR_INVALID;
    if (n_rays >= (1ull << 36) || n_norm >= (1ull << 36)) return KNERF_ERR_INVALID;
    if (n_rays == 0) return KNERF_OK;
    a.rec = static_cast<const uint4*>(field->records); a.brick_of = field->brick_of; a.bits = field->bits;
    a.L = field->brick_log2; a.By = B[1]; a.Bz = B[2]; a.n_bricks = (long long)field->n_bricks;
    a.o = origins; a.d = directions; a.near = near; a.far = far; a.near0 = near_all; a.far0 = far_all; a.target = target;
    a.n = (long long)n_rays; a.step = step; a.eps = termination;
    a.gscale = (float)(2.0 / (3.0 * (double)(n_norm ? n_norm : n_rays)));
    a.white = (flags & KNERF_BAKED_WHITE_BACKGROUND) ? 1 : 0;
    a.grad = train->grad; a.sq_err = sq_err;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipErrorInvalidValue;
    switch (deg * 8 + lanes) {
        case 0 * 8 + 1: e = bricks_train::launch_rays<0, 1>(a, s); break;
        case 1 * 8 + 1: e = bricks_train::launch_rays<1, 1>(a, s); break;
        case 1 * 8 + 2: e = bricks_train::launch_rays<1, 2>(a, s); break;
        case 2 * 8 + 1: e = bricks_train::launch_rays<2, 1>(a, s); break;
        case 2 * 8 + 4: e = bricks_train::launch_rays<2, 4>(a, s); break;
        case 3 * 8 + 1: e = bricks_train::launch_rays<3, 1>(a, s); break;
        case 3 * 8 + 4: e = bricks_train::launch_rays<3, 4>(a, s); break;
        default: return KNERF_ERR_INVALID;
    }
    return e == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_bricks_train_apply(void* stream, const knerf_baked_bricks_train* train, const uint8_t* flags, float* master,
                                              float* m, float* v, float rate_sigma, float rate_sh, float beta_1, float beta_2,
                                              float epsilon) {
    int B[3];
    double scale[3];
    unsigned long long n_records = 0;
    if (!bricks_train::check_state(train, B, scale, n_records) || !flags || !master || !m || !v) return KNERF_ERR_INVALID;
    if (!std::isfinite(rate_sigma) || !std::isfinite(rate_sh) || !(beta_1 >= 0.f && beta_1 < 1.f) || !(beta_2 >= 0.f && beta_2 < 1.f) ||
        !(epsilon > 0.f) || !std::isfinite(epsilon))
        return KNERF_ERR_INVALID;
    const int deg = train->field.sh_degree;
    bricks_train::ApplyArgs a{};
    a.rec = static_cast<uint4*>(const_cast<void*>(train->field.records));
    a.flags = flags; a.w = master; a.m = m; a.v = v; a.g = train->grad;
    a.n_records = (long long)n_records;
    a.K = bricks_train::n_coeff(deg); a.nch = bricks_train::rec_bytes(deg) / 16;
    a.rate_sigma = rate_sigma; a.rate_sh = rate_sh; a.b1 = beta_1; a.b2 = beta_2; a.eps = epsilon;
    const unsigned long long blocks = (n_records * (unsigned)a.nch + 255) / 256;
    if (blocks >= (1ull << 31)) return KNERF_ERR_INVALID;
    hipLaunchKernelGGL(bricks_train::baked_bricks_train_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
