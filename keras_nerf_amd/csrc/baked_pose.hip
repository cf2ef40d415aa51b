// baked_pose.hip -- how the baked-field objective moves when a ray moves (gfx950), context-free: the gradient of the loss of
// baked_train.hip with respect to every ray's origin and direction, for dense and for brick fields, and the reduction of those per-ray
// gradients to one rigid-motion gradient per camera.  Extension: the reference has nothing of the kind (BARF, NeRF-- and every current
// toolkit refine their cameras with the field in this way).  include/knerf.h holds the contract; tests/baked_pose_reference.py is its
// fp64 restatement; DESIGN.md 2.24 has the derivation.  What the file shares with the other baked*.hip files is in baked_common.h.
//
//   baked_ray_gradients_kernel  <DEG, G, BRICK>, the lane variants of baked_train_rays_kernel: G lanes march one ray, lane `sub` owns chunks
//                             sub, sub + G, ... of every record.  The two marches are those of baked_train.hip sample for sample: the
//                             first gives C, O and g = dL/dout, the second recomputes every sample and forms dL/dsigma_j and dL/dr_jc
//                             with total minus prefix.  Where the train kernel scatters them to the 8 corners, this one keeps them on
//                             the ray.  The field is trilinear inside a cell, so with fr the fractions of locate
//                                 d sigma / d fr_a = sum_n (d tau_n / d fr_a) sigma_n,   d r_c / d fr_a = sum_n (d tau_n / d fr_a) r_nc,
//                             r_nc = sum_k Y_k coef_nkc the colour of corner n alone, d tau_n / d fr_a the weight with the factor of axis a
//                             replaced by +-1.  Every lane forms these sums over ITS chunks (sigma lives in lane 0's first chunk) and
//                             adds   G_ja = dsig_j dsigma/dfr_a + sum_c dr_jc dr_c/dfr_a   to its own accumulators (plain and times t_j);
//                             nothing crosses lanes inside the march.  Also per lane:  q[k][c] += dr_jc cf_jkc  over its own elements
//                             (for the basis' dependence on the direction) and  sum_j dsig_j sigma_j  (for delta = step |d|).
//                             At the ray's end the group adds its lanes up (DPP), and lane 0 stores
//                                 grad_origin    = scale * sum_j G_j
//                                 grad_direction = scale * sum_j t_j G_j + (sum_j dsig_j sigma_j) (step / delta) u
//                                                  + (1 / |d|) (I - u u^T) sum_kc q[k][c] grad Y_k(u)
//                             once: no atomics, no scratch buffer.  A ray that misses, has |d| = 0 or an all-zero g stores zeros.
//                             BRICK: a corner's record address goes through brick_of as in baked_train.hip (an entry < 0 or >= n_bricks
//                             counts as absent before any address is formed and reads as a zero record); nothing else differs, so a brick
//                             field gives the bits of its dense field.
//   pose_gradients_kernel     one block per view: the lanes stride over ALL rays in a fixed order, add those of their view in double
//                             (tau: grad_origin; omega: d x grad_direction) and the block adds its 256 partial sums in a fixed tree.
//                             No atomics: two launches on the same inputs give the same bits.  A view index outside [0, V) matches no
//                             block and is never written through.
#include "baked_common.h"

namespace knerf {
namespace baked_pose {
using namespace baked;

struct PoseArgs {
    const uint4* rec;
    const int* brick_of;                            // BRICK only
    const unsigned* bits;
    int R[3];
    int L, By, Bz;                                  // BRICK only: log2 of the brick edge; the brick grid's y and z extents
    long long n_bricks;
    float lo[3], hi[3], scale[3];
    const float *o, *d, *near, *far, *target;
    float near0, far0;
    long long n;
    float step, eps, gscale;                        // gscale = 2 / (3 N)
    int white;
    float *grad_o, *grad_d, *sq_err;
};

// the gradient of the polynomials of sh_eval as they are written (their extension off the sphere; the caller projects it away): D[k] = (d/dx, d/dy, d/dz)
template <int DEG>
__device__ __forceinline__ void sh_grad(float x, float y, float z, float (&D)[n_coeff(DEG)][3]) {
#pragma unroll
    for (int k = 0; k < n_coeff(DEG); ++k) D[k][0] = D[k][1] = D[k][2] = 0.f;
    if constexpr (DEG >= 1) {
        D[1][1] = 0.4886025119029199f;
        D[2][2] = 0.4886025119029199f;
        D[3][0] = 0.4886025119029199f;
    }
    if constexpr (DEG >= 2) {
        const float a = 1.0925484305920792f, b = 0.31539156525252005f, e = 0.5462742152960396f;
        D[4][0] = a * y; D[4][1] = a * x;
        D[5][1] = a * z; D[5][2] = a * y;
        D[6][2] = 6.f * b * z;
        D[7][0] = a * z; D[7][2] = a * x;
        D[8][0] = 2.f * e * x; D[8][1] = -2.f * e * y;
        if constexpr (DEG >= 3) {
            const float xx = x * x, yy = y * y, zz = z * z;
            const float f = 0.5900435899266435f, g = 2.890611442640554f, h = 0.4570457994644658f, p = 0.3731763325901154f,
                        q = 1.445305721320277f;
            D[9][0] = 6.f * f * (x * y); D[9][1] = 3.f * f * (xx - yy);
            D[10][0] = g * (y * z); D[10][1] = g * (x * z); D[10][2] = g * (x * y);
            D[11][1] = h * (5.f * zz - 1.f); D[11][2] = 10.f * h * (y * z);
            D[12][2] = p * (15.f * zz - 3.f);
            D[13][0] = h * (5.f * zz - 1.f); D[13][2] = 10.f * h * (x * z);
            D[14][0] = 2.f * q * (x * z); D[14][1] = -2.f * q * (y * z); D[14][2] = q * (xx - yy);
            D[15][0] = 3.f * f * (xx - yy); D[15][1] = -6.f * f * (x * y);
        }
    }
}

// what the second march needs from the first: g = dL/dout (already gated by the output clamp) and the totals
struct Totals {
    float g[3], img[3], opa, bg;
};

// what the second march leaves on a lane: sums over the ray's samples, over this lane's chunks where a record enters
template <int DEG, int G>
struct Sums {
    float go[3];                                    // sum_j G_j, before the scale
    float gt[3];                                    // sum_j t_j G_j
    float sds;                                      // sum_j dsig_j sigma_j (the same on every lane of the group)
    float q[(rec_bytes(DEG) / 16 + G - 1) / G][8];  // sum_j dr_jc cf_jkc in the lane's own element order
};

// One march of one ray over the samples [i, i1), as march of baked_train.hip.  BWD = false: img / opa end as C / O.  BWD = true: the same
// arithmetic again (img / opa are then the prefix sums), and per sample the ray's sums grow.  rot = (2 sub) mod 3: element s of chunk
// sub + j G is column 8 (sub + j G) - 2 + s of [k][c], so its channel is (rot + (8 j G - 2 + s)) mod 3.
template <int DEG, int G, bool BRICK, bool BWD>
__device__ __forceinline__ void march(const PoseArgs& a, const float (&o3)[3], const float (&d3)[3], float near, int i, int i1,
                                      float delta, int sub, int rot, const float (&Y)[n_coeff(DEG)],
                                      const float (&wr)[(rec_bytes(DEG) / 16 + G - 1) / G][8],
                                      const float (&wg)[(rec_bytes(DEG) / 16 + G - 1) / G][8],
                                      const float (&wb)[(rec_bytes(DEG) / 16 + G - 1) / G][8], float (&img)[3], float& opa, const Totals& tt,
                                      Sums<DEG, G>& sums) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, CPL = (NCH + G - 1) / G;
    [[maybe_unused]] const long long sy = a.R[2], sx = (long long)a.R[1] * a.R[2];
    const int cyc = a.R[1] - 1, czc = a.R[2] - 1;
    [[maybe_unused]] const int L = a.L, inm = (1 << L) - 1;
    [[maybe_unused]] int last_key = -1, last_slot = -1;     // BRICK: the brick this lane looked up last, as baked.hip
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
            // a corner's record index, or -1 for a point of an absent brick (BRICK only: through the table, with the lane's one-entry
            // cache of the brick it looked up last, as baked.hip).  A record's index fits 32 bits (n_bricks <= Bx By Bz, so
            // at most 1032^3 records); byte offsets are formed in 64
            [[maybe_unused]] const long long base = (long long)ci[0] * sx + (long long)ci[1] * sy + ci[2];
            auto record_of = [&](int cn) -> long long {
                if constexpr (BRICK) {
                    const int x = ci[0] + ((cn >> 2) & 1), y = ci[1] + ((cn >> 1) & 1), z = ci[2] + (cn & 1);
                    const int key = ((x >> L) * a.By + (y >> L)) * a.Bz + (z >> L);
                    const int slot = key == last_key ? last_slot : a.brick_of[key];
                    last_key = key; last_slot = slot;
                    const int in = ((((x & inm) << L) | (y & inm)) << L) | (z & inm);
                    const bool stored = slot >= 0 && (long long)slot < a.n_bricks;
                    return stored ? (long long)(int)(((unsigned)slot << (3 * L)) + (unsigned)in) : -1;
                } else {
                    return base + ((cn & 4) ? sx : 0) + ((cn & 2) ? sy : 0) + (cn & 1);
                }
            };
            float sig = 0.f, cf[CPL][8];
#pragma unroll
            for (int j = 0; j < CPL; ++j)
#pragma unroll
                for (int s = 0; s < 8; ++s) cf[j][s] = 0.f;
            float dsg[3] = {0.f, 0.f, 0.f}, dcol[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};     // [axis], [axis][channel]
            // The one-lane variants of degree 2 and 3 walk the corners of the SECOND march in a loop that stays a loop: unrolled, hipcc
            // keeps the halfs of all 8 corners live for the two sums they enter (cf and the corner's own colour) beside the ray's
            // sums, and the kernel leaves the register file (degree 3: 584 bytes of scratch per lane).  The arithmetic is the same.
            constexpr int kCornerUnroll = (BWD && G == 1 && DEG >= 2) ? 1 : 8;
            // BRICK, unrolled: the 8 addresses in front of the loads, so that the loads issue together; the table is then read against
            // the brick of the sample BEFORE, as baked.hip does, and the 8 lookups do not wait for each other (measured on an
            // MI355X at 256^3, degree 2: 3.7 against 5.5 ms a launch).  The dense address is plain arithmetic and is formed at its
            // load: put in front as well it cost time (3.8 against 3.0 ms)
            constexpr bool kInFront = BRICK && kCornerUnroll == 8;
            [[maybe_unused]] long long at[8];
            if constexpr (kInFront) {
                int key[8], slot[8];
#pragma unroll
                for (int cn = 0; cn < 8; ++cn) {
                    const int x = ci[0] + ((cn >> 2) & 1), y = ci[1] + ((cn >> 1) & 1), z = ci[2] + (cn & 1);
                    key[cn] = ((x >> L) * a.By + (y >> L)) * a.Bz + (z >> L);
                }
#pragma unroll
                for (int cn = 0; cn < 8; ++cn) slot[cn] = key[cn] == last_key ? last_slot : a.brick_of[key[cn]];
                last_key = key[0]; last_slot = slot[0];
#pragma unroll
                for (int cn = 0; cn < 8; ++cn) {
                    const int x = ci[0] + ((cn >> 2) & 1), y = ci[1] + ((cn >> 1) & 1), z = ci[2] + (cn & 1);
                    const int in = ((((x & inm) << L) | (y & inm)) << L) | (z & inm);
                    const bool stored = slot[cn] >= 0 && (long long)slot[cn] < a.n_bricks;
                    at[cn] = stored ? (long long)(int)(((unsigned)slot[cn] << (3 * L)) + (unsigned)in) : -1;
                }
            }
#pragma unroll kCornerUnroll
            for (int cn = 0; cn < 8; ++cn) {
                const float w = ((cn & 4) ? fr[0] : 1.f - fr[0]) * ((cn & 2) ? fr[1] : 1.f - fr[1]) * ((cn & 1) ? fr[2] : 1.f - fr[2]);
                long long pt;
                if constexpr (kInFront) pt = at[cn]; else pt = record_of(cn);
                uint4 v[CPL];
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const int qc = sub + j * G;
                    v[j] = (qc < NCH && pt >= 0) ? a.rec[pt * NCH + qc] : make_uint4(0u, 0u, 0u, 0u);
                }
                float rn[3] = {0.f, 0.f, 0.f}, sn = 0.f;            // BWD: this corner's colour over the lane's chunks, and its sigma
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const unsigned wd[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                    const bool first = j == 0 && sub == 0;
                    if (j == 0) {
                        sn = first ? __uint_as_float(wd[0]) : 0.f;
                        sig = __builtin_fmaf(w, sn, sig);
                    }
#pragma unroll
                    for (int s = 0; s < 8; ++s) {
                        const float hv = half_bits_to_float(wd[s >> 1] >> ((s & 1) * 16));
                        cf[j][s] = __builtin_fmaf(w, hv, cf[j][s]);
                        if constexpr (BWD) {
                            if constexpr (G == 1) {
                                const int e = 8 * j - 2 + s;
                                if (e >= 0 && e < 3 * K) rn[e % 3] = __builtin_fmaf(hv, Y[e / 3], rn[e % 3]);
                            } else {
                                const int e = 8 * (sub + j * G) - 2 + s;
                                const float hm = (e >= 0 && e < 3 * K) ? hv : 0.f;      // sigma's bytes and the padding are no coefficients
                                rn[0] = __builtin_fmaf(hm, wr[j][s], rn[0]);
                                rn[1] = __builtin_fmaf(hm, wg[j][s], rn[1]);
                                rn[2] = __builtin_fmaf(hm, wb[j][s], rn[2]);
                            }
                        }
                    }
                }
                if constexpr (BWD) {
                    const float wx = (cn & 4) ? fr[0] : 1.f - fr[0], wy = (cn & 2) ? fr[1] : 1.f - fr[1], wz = (cn & 1) ? fr[2] : 1.f - fr[2];
                    const float dw[3] = {(cn & 4) ? wy * wz : -(wy * wz), (cn & 2) ? wx * wz : -(wx * wz), (cn & 1) ? wx * wy : -(wx * wy)};
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        dsg[ax] = __builtin_fmaf(dw[ax], sn, dsg[ax]);
#pragma unroll
                        for (int c = 0; c < 3; ++c) dcol[ax][c] = __builtin_fmaf(dw[ax], rn[c], dcol[ax][c]);
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
                    for (int ax = 0; ax < 3; ++ax) {
                        float gj = dsig * dsg[ax];
#pragma unroll
                        for (int c = 0; c < 3; ++c) gj = __builtin_fmaf(dr[c], dcol[ax][c], gj);
                        sums.go[ax] = sums.go[ax] + gj;
                        sums.gt[ax] = __builtin_fmaf(t, gj, sums.gt[ax]);
                    }
                    sums.sds = __builtin_fmaf(dsig, sig, sums.sds);
                    // dr by the channel of the lane's elements: drr[m] = dr[(m + rot) mod 3]
                    const float drr[3] = {rot == 0 ? dr[0] : (rot == 1 ? dr[1] : dr[2]), rot == 0 ? dr[1] : (rot == 1 ? dr[2] : dr[0]),
                                          rot == 0 ? dr[2] : (rot == 1 ? dr[0] : dr[1])};
#pragma unroll
                    for (int j = 0; j < CPL; ++j) {
#pragma unroll
                        for (int s = 0; s < 8; ++s) {
                            constexpr int kOff = 3 * 64 - 2;                // keeps the remainder's operand positive
                            sums.q[j][s] = __builtin_fmaf(drr[(8 * j * G + s + kOff) % 3], cf[j][s], sums.q[j][s]);
                        }
                    }
                }
            }
            if (a.eps > 0.f && T < a.eps) { done = true; break; }
        }
    }
}

template <int DEG, int G, bool BRICK>
__global__ __launch_bounds__(kBlock) void baked_ray_gradients_kernel(PoseArgs a) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, CPL = (NCH + G - 1) / G;
    static_assert(G == 1 || G == 2 || G == 4, "a group is a lane, a pair or a quad");
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long ray = gid / G;
    const int sub = (int)(gid & (G - 1));
    const int rot = (2 * sub) % 3;
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
    Sums<DEG, G> sums{};
    march<DEG, G, BRICK, false>(a, o3, d3, near, i0, i1, delta, sub, rot, Y, wr, wg, wb, tt.img, tt.opa, tt, sums);
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
    float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
    if (any && nrm > 0.f) {                                 // the same on every lane of the group
        float img[3], opa;
        march<DEG, G, BRICK, true>(a, o3, d3, near, i0, i1, delta, sub, rot, Y, wr, wg, wb, img, opa, tt, sums);
        // the basis' share: sum over the lane's elements of q[k][c] grad Y_k(u), then over the group
        float D[K][3];
        sh_grad<DEG>(ux, uy, uz, D);
        float vy[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int e = 8 * (sub + j * G) - 2 + s;
                const int k = e / 3;
#pragma unroll
                for (int kk = 0; kk < K; ++kk) {
                    const bool own = e >= 0 && k == kk;     // elements outside [k][c] hold q = 0 and own no k
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) vy[ax] = own ? __builtin_fmaf(sums.q[j][s], D[kk][ax], vy[ax]) : vy[ax];
                }
            }
        }
        const float u3[3] = {ux, uy, uz};
        float along = 0.f;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            vy[ax] = group_sum<G>(vy[ax]);
            along = __builtin_fmaf(u3[ax], vy[ax], along);
        }
        const float stretch = sums.sds * (a.step / delta);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            go[ax] = group_sum<G>(sums.go[ax]) * a.scale[ax];
            gd[ax] = group_sum<G>(sums.gt[ax]) * a.scale[ax] + stretch * u3[ax] + (vy[ax] - u3[ax] * along) / nrm;
        }
    }
    if (sub == 0) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            a.grad_o[ray * 3 + ax] = go[ax];
            a.grad_d[ray * 3 + ax] = gd[ax];
        }
    }
}

template <bool BRICK>
hipError_t launch_rays(int deg, int lanes, const PoseArgs& a, hipStream_t s) {
    return dispatch_deg_lanes(deg, lanes, [&](auto DEG, auto G) {
        const long long blocks = (a.n * G + kBlock - 1) / kBlock;
        hipLaunchKernelGGL((baked_ray_gradients_kernel<DEG, G, BRICK>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
        return hipGetLastError();
    });
}

// the lattice of either field struct: what knerf_baked_render refuses of it, and the scale of locate
static bool check_field(const void* records, const unsigned* bits, const int32_t (&res)[3], int deg, const float (&lo)[3],
                        const float (&hi)[3], PoseArgs& a) {
    unsigned long long points = 0;
    if (!records || !bits || !check_lattice(res, lo, hi, deg, a.scale, points)) return false;
    for (int c = 0; c < 3; ++c) { a.R[c] = res[c]; a.lo[c] = lo[c]; a.hi[c] = hi[c]; }
    return true;
}

// the ray arguments of knerf_baked_train_rays, checked as there; lanes comes back resolved.  n_rays = 0 is for the caller
static bool check_pose_rays(int deg, const float* origins, const float* directions, const float* near, const float* far, float near_all,
                            float far_all, const float* target, uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags,
                            float* grad_origin, float* grad_direction, float* sq_err, PoseArgs& a, int& lanes) {
    if (!origins || !directions || !target || !grad_origin || !grad_direction) return false;
    if (!check_rays(near, far, near_all, far_all, n_rays, step, termination, flags) || n_norm >= (1ull << 36)) return false;
    lanes = pick_lanes(deg, flags, kLaneGroups);
    if (!lanes) return false;
    a.o = origins; a.d = directions; a.near = near; a.far = far; a.near0 = near_all; a.far0 = far_all; a.target = target;
    a.n = (long long)n_rays; a.step = step; a.eps = termination;
    a.gscale = (float)(2.0 / (3.0 * (double)(n_norm ? n_norm : (n_rays ? n_rays : 1))));
    a.white = (flags & KNERF_BAKED_WHITE_BACKGROUND) ? 1 : 0;
    a.grad_o = grad_origin; a.grad_d = grad_direction; a.sq_err = sq_err;
    return true;
}

constexpr int kPoseBlock = 256;

__global__ __launch_bounds__(kPoseBlock) void pose_gradients_kernel(const float* go, const float* gd, const float* d, const int* view,
                                                                     long long n, double* out) {
    const int v = (int)blockIdx.x, tid = (int)threadIdx.x;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long i = tid; i < n; i += kPoseBlock) {
        if (view[i] != v) continue;
        const double ax = go[i * 3 + 0], ay = go[i * 3 + 1], az = go[i * 3 + 2];
        const double bx = gd[i * 3 + 0], by = gd[i * 3 + 1], bz = gd[i * 3 + 2];
        const double dx = d[i * 3 + 0], dy = d[i * 3 + 1], dz = d[i * 3 + 2];
        s[0] += ax; s[1] += ay; s[2] += az;
        s[3] += dy * bz - dz * by;                       // d x grad_direction; the products of two floats are exact in double
        s[4] += dz * bx - dx * bz;
        s[5] += dx * by - dy * bx;
    }
    __shared__ double part[6][kPoseBlock];
#pragma unroll
    for (int k = 0; k < 6; ++k) part[k][tid] = s[k];
    __syncthreads();
    for (int h = kPoseBlock / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < 6; ++k) part[k][tid] = part[k][tid] + part[k][tid + h];
        }
        __syncthreads();
    }
    if (tid < 6) out[(long long)v * 6 + tid] = part[tid][0];
}

}  // namespace baked_pose
}  // namespace knerf

using namespace knerf;

extern "C" int knerf_baked_ray_gradients(void* stream, const knerf_baked_field* field, const float* origins, const float* directions,
                                         const float* near, const float* far, float near_all, float far_all, const float* target,
                                         uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* grad_origin,
                                         float* grad_direction, float* sq_err) {
    baked_pose::PoseArgs a{};
    int lanes = 0;
    if (!field || !baked_pose::check_field(field->records, field->bits, field->resolution, field->sh_degree, field->lo, field->hi, a))
        return KNERF_ERR_INVALID;
    if (!baked_pose::check_pose_rays(field->sh_degree, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step,
                                     termination, flags, grad_origin, grad_direction, sq_err, a, lanes))
        return KNERF_ERR_INVALID;
    if (n_rays == 0) return KNERF_OK;
    a.rec = static_cast<const uint4*>(field->records); a.bits = field->bits;
    const hipError_t e = baked_pose::launch_rays<false>(field->sh_degree, lanes, a, (hipStream_t)stream);
    return e == hipSuccess ? KNERF_OK : (e == hipErrorInvalidValue ? KNERF_ERR_INVALID : KNERF_ERR_HIP);
}

extern "C" int knerf_baked_ray_gradients_bricks(void* stream, const knerf_baked_bricks* field, const float* origins,
                                                const float* directions, const float* near, const float* far, float near_all, float far_all,
                                                const float* target, uint64_t n_rays, uint64_t n_norm, float step, float termination,
                                                int flags, float* grad_origin, float* grad_direction, float* sq_err) {
    baked_pose::PoseArgs a{};
    int lanes = 0, B[3];
    if (!field || !field->brick_of ||
        !baked_pose::check_field(field->records, field->bits, field->resolution, field->sh_degree, field->lo, field->hi, a))
        return KNERF_ERR_INVALID;
    const int deg = field->sh_degree;
    if (!baked::check_brick_grid(field->resolution, deg, field->brick_log2, field->n_bricks, B)) return KNERF_ERR_INVALID;
    if (!baked_pose::check_pose_rays(deg, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination,
                                     flags, grad_origin, grad_direction, sq_err, a, lanes))
        return KNERF_ERR_INVALID;
    if (n_rays == 0) return KNERF_OK;
    a.rec = static_cast<const uint4*>(field->records); a.brick_of = field->brick_of; a.bits = field->bits;
    a.L = field->brick_log2; a.By = B[1]; a.Bz = B[2]; a.n_bricks = (long long)field->n_bricks;
    const hipError_t e = baked_pose::launch_rays<true>(deg, lanes, a, (hipStream_t)stream);
    return e == hipSuccess ? KNERF_OK : (e == hipErrorInvalidValue ? KNERF_ERR_INVALID : KNERF_ERR_HIP);
}

extern "C" int knerf_pose_gradients(void* stream, const float* grad_origin, const float* grad_direction, const float* directions,
                                    const int32_t* view, uint64_t n_rays, uint64_t n_views, double* out) {
    if (!grad_origin || !grad_direction || !directions || !view || !out) return KNERF_ERR_INVALID;
    if (n_rays >= (1ull << 36) || n_views >= (1ull << 31)) return KNERF_ERR_INVALID;
    if (n_views == 0) return KNERF_OK;
    hipLaunchKernelGGL(baked_pose::pose_gradients_kernel, dim3((unsigned)n_views), dim3(baked_pose::kPoseBlock), 0, (hipStream_t)stream,
                       grad_origin, grad_direction, directions, view, (long long)n_rays, out);
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
