// baked_train.hip -- optimising a baked field against ray batches (gfx950), context-free: the gradient of the march of baked.hip and
// the Adam step that rewrites the records, for dense and for brick storage (the dense record table of a brick field is never formed).
// Extension: the reference has nothing of the kind (PlenOctrees and Plenoxels optimise their grids against the photographs after
// conversion in this way).  include/knerf.h holds the contract; tests/baked_train_reference.py is its fp64 restatement.  What the file
// shares with the other baked*.hip files is in baked_common.h.
//
//   baked_train_rays_kernel   <DEG, G, Args>, the lane variants of baked_render_kernel: G lanes march one ray, lane `sub` owns chunks
//                             sub, sub + G, ... of every record.  Each ray is marched TWICE in the one launch by the same code
//                             (march<DEG, G, BWD>): the first march is the render kernel's arithmetic sample for sample and gives C, O
//                             and with them g = dL/dout; the second recomputes every sample, forms dL/dsigma and dL/dr and adds them
//                             to the gradient rows of the sample's 8 corners with float atomics.
//                             The sum over LATER samples that dL/dsigma needs is total minus prefix, per channel:
//                                 sum_{i>j} w_i A_i = sum_c g_c ((C_c - P_c(j)) - bg (O - P_O(j))),
//                             P the running sums of the second march.  They are the first march's own arithmetic, so at a ray's last
//                             sample P equals the total bit for bit and the suffix is exactly 0; in between the difference carries the
//                             rounding of the totals, about 2^-24 |C|.
//                             Args = TrainArgs (dense) or BrickTrainArgs: ONE march for both storages (tests/test_gpu_baked_bricks_train.py
//                             holds the two bit for bit).  Only a corner's address and its row differ (Args::kBrick).  Dense: the row
//                             of a lattice point is slot_of[point].  Brick: the address is formed through brick_of as in
//                             baked_render_kernel, with the lane's one-entry cache of the brick it looked up last; an entry < 0 or
//                             >= n_bricks counts as absent BEFORE any address is formed, an absent corner's record reads as zero and
//                             NOTHING is added for it, so a damaged table never becomes an out-of-range read or write.  There is no slot
//                             table: the rows of gradient, master value and moments are per STORED RECORD, and a row's index is the
//                             record's index.
//                             Args::kExt (Ext<TrainArgs>, Ext<BrickTrainArgs>): the same march and kernel under the objective record of
//                             knerf_baked_train_rays_ext -- the robust losses and the distortion / opacity-entropy regularisers of a
//                             ray's weights.  The first march also keeps the prefix sums D needs, the second forms
//                             r_j = wd dD/dw_j + we dH/dw, adds it to A_j and takes the later samples' share as total minus a running
//                             prefix; the early exit of a ray with g = 0 holds only where no regulariser has a gradient.  Every line
//                             of it stands under `if constexpr`: the plain instantiations are instruction for instruction what they
//                             were.  tests/baked_objective_reference.py restates it in fp64.
//                             Args::kRgba (Rgba<TrainArgs>, Rgba<BrickTrainArgs>): the extended kernel against RGBA photographs
//                             (knerf_baked_train_rays_rgba) -- a background per ray where the flag's colour is
//                             otherwise, the target recomposited over it with the photograph's alpha, and the opacity loss
//                             (lambda_o / N)(O - alpha)^2, a function of O alone that enters r_j and the total like the entropy term.
//                             Every line of it stands under `if constexpr (RGBA)`; tests/baked_rgba_reference.py restates it in fp64.
//                             Args::kDepth (Depth<TrainArgs>, Depth<BrickTrainArgs>): the rgba kernel with depth supervision
//                             (knerf_baked_train_rays_depth) -- the first march also sums Z = sum w_j t_j, the render
//                             kernel's depth bit for bit, and the term (lambda_z / N) c (Z - z*)^2, linear in the weights through Z,
//                             enters r_j as zeta t_j and the total as zeta Z, zeta = (lambda_z / N) 2 c (Z - z*).  Every line of it
//                             stands under `if constexpr (DEPTH)`; tests/baked_depth_reference.py restates it in fp64.
//   Gradient rows: fp32 [n_slots][1 + 3 K], sigma first, then [k][c]: the columns of a record.  Every lane of a group holds the whole
//   basis and the same dL/dr and dL/dsigma, so any lane can form any column: lane `sub` adds the columns sub, sub + G, ... of a
//   corner's row, so that ONE atomic instruction of the group adds G consecutive floats (the memory side works in 64-byte requests;
//   with the columns dealt out by record chunk an instruction touched both 64-byte halves of every row: 19.5 against 7.6 ms a launch).
//   baked_train_apply_kernel  one lane per (slot, chunk): Keras-form Adam on the chunk's columns (m += (g - m)(1 - b1),
//                             v += (g g - v)(1 - b2), w -= rate m / (sqrt(v) + eps)), sigma masked by the slot's flag and projected
//                             to >= 0, the chunk of the record rewritten (fp32 sigma, fp16 coefficients to nearest even, zero padding),
//                             the gradient columns zeroed.
//   baked_bricks_train_apply_kernel  one lane per (record, chunk): the same arithmetic on the rows of a brick field.  flags[record]
//                             bit 0: the record is a slot (a corner of a support cell); a record without it is skipped entirely.
//                             Bit 1: sigma is trainable there.
#include "baked_common.h"

namespace knerf {
namespace baked_train {
using namespace baked;

struct TrainArgs {
    static constexpr bool kBrick = false, kExt = false, kRgba = false, kDepth = false;
    const uint4* rec;
    const unsigned* bits;
    int R[3];
    float lo[3], hi[3], scale[3];
    const float *o, *d, *near, *far, *target;
    float near0, far0;
    long long n;
    float step, eps, gscale;                        // gscale = 2 / (3 N)
    int white;
    const int* slot_of;
    long long n_slots;
    float* grad;
    float* sq_err;
};

struct BrickTrainArgs {
    static constexpr bool kBrick = true, kExt = false, kRgba = false, kDepth = false;
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

// The extended objective (knerf_baked_train_rays_ext): the argument struct of a storage with the objective behind it.
// Args::kExt is the ONE compile-time switch of march and kernel; every line it adds stands under `if constexpr (Args::kExt)`, so the
// plain instantiations are the text they were.  Kind and weights are run-time values: one extended instantiation per <DEG, G, storage>.
struct Objective {
    int kind;                                       // KNERF_LOSS_*
    float huber_delta;
    float hscale;                                   // 1 / (3 N): g_c = rho'(d_c) hscale (for mse the bits of diff * gscale)
    float wd, we;                                   // lambda_d / N, lambda_e / N
    float* terms;                                   // [n][4] ([n][5] under kRgba, [n][6] under kDepth) or NULL
};
template <class Base>
struct Ext : Base {
    static constexpr bool kExt = true;
    Objective obj;
};

// Per-ray backgrounds and alpha targets (knerf_baked_train_rays_rgba): the extended argument struct with the rgba record
// behind it.  Args::kRgba is the second compile-time switch; every line it adds stands under `if constexpr (Args::kRgba)` (RGBA), so the
// plain and the extended instantiations are the text they were.  One rgba instantiation per <DEG, G, storage>.
struct RgbaArgs {
    const float* background;                        // [n][3] or NULL: the flag's colour on every channel
    const float* alpha;                             // [n] or NULL: every alpha reads as 1 and the target is used as it is
    float stored;                                   // 0 or 1: what the target's rgb is composited over
    float wo;                                       // lambda_o / N
};
template <class Base>
struct Rgba : Ext<Base> {
    static constexpr bool kRgba = true;
    RgbaArgs rgba;
};

// Depth supervision (knerf_baked_train_rays_depth): the rgba argument struct with the depth record behind it.
// Args::kDepth is the third compile-time switch; every line it adds stands under `if constexpr (Args::kDepth)` (DEPTH), so the plain, the
// extended and the rgba instantiations are the text they were.  One depth instantiation per <DEG, G, storage>.
struct DepthArgs {
    const float* target;                            // [n]: z*, in ray-parameter units (what baked_render_kernel writes as depth)
    const float* weight;                            // [n] >= 0 or NULL: every ray 1
    float wz;                                       // lambda_z / N
};
template <class Base>
struct Depth : Rgba<Base> {
    static constexpr bool kDepth = true;
    DepthArgs depth;
};

// kExt: what the regularisers keep per ray, with m_j = (i_j - first) delta and the exclusive prefixes W_k = sum_{j<k} w_j (the march's own
// opa) and M_k = sum_{j<k} w_j m_j.  First march: M ends as MT, S1 = sum w_k (m_k W_k - M_k), S2 = sum w_k^2, so D = 2 S1 + delta S2 / 3.
// Second march: M runs again as the prefix, run = sum_{i<=j} w_i r_i, r_j = wd dD/dw_j + re the regularisers' share of A_j; the later
// samples' share is total - run, total = wd 2 D + re O (D is homogeneous of degree 2 in w, H depends on O alone).
struct RegState {
    float M, S1, S2, run;
    int first;                                      // index of the ray's first fetched sample, -1: none yet
    float mt, wd, re, total;                        // MT, lambda_d / N, (lambda_e / N) dH/dw, sum_i w_i r_i
    float Z, zeta;                                  // kDepth: Z = sum_j w_j t_j of the first march; zeta = (lambda_z / N) 2 c (Z - z*)
};

// what the second march needs from the first: g = dL/dout (already gated by the output clamp) and the totals
struct Totals {
    float g[3], img[3], opa, bg;
    float b3[3];                                    // kRgba: the ray's background per channel, used where bg is otherwise
};

// One march of one ray over the samples [i, i1): the loop of baked_render_kernel without statistics (and without depth but under kDepth).  BWD = false: img / opa
// end as C / O.  BWD = true: the same arithmetic again (img / opa are then the prefix sums), and per sample the gradient is added.
template <int DEG, int G, bool BWD, class Args>
__device__ __forceinline__ void march(const Args& a, const float (&o3)[3], const float (&d3)[3], float near, int i, int i1,
                                      float delta, int sub, const float (&Y)[n_coeff(DEG)],
                                      const float (&wr)[(rec_bytes(DEG) / 16 + G - 1) / G][8],
                                      const float (&wg)[(rec_bytes(DEG) / 16 + G - 1) / G][8],
                                      const float (&wb)[(rec_bytes(DEG) / 16 + G - 1) / G][8],
                                      const float (&gy)[(1 + 3 * n_coeff(DEG) + G - 1) / G][3], float (&img)[3], float& opa, const Totals& tt,
                                      [[maybe_unused]] RegState& rs) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, CPL = (NCH + G - 1) / G, W = 1 + 3 * K, NI = (W + G - 1) / G;
    constexpr bool BRICK = Args::kBrick, EXT = Args::kExt, RGBA = Args::kRgba, DEPTH = Args::kDepth;
    [[maybe_unused]] const long long sy = a.R[2], sx = (long long)a.R[1] * a.R[2];     // dense: the lattice's strides
    const int cyc = a.R[1] - 1, czc = a.R[2] - 1;
    [[maybe_unused]] const int L = brick_log2(a), inm = (1 << L) - 1;
    [[maybe_unused]] int last_key = -1, last_slot = -1;     // BRICK: the brick this lane looked up last, as baked_render_kernel
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
            // dense: the address is formed at its load.  BRICK: the 8 corner records through the brick table, in front of the loads:
            // at[cn] < 0 = a point of an absent brick; the 8 record indices stay live from the loads to the scatter
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
                // a record's index fits 32 bits (n_bricks <= Bx By Bz, so at most 1032^3 records); byte offsets are formed in 64
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
            [[maybe_unused]] float mk = 0.f, Wk = 0.f, Mk = 0.f;    // EXT: m_k and the exclusive prefixes W_k, M_k
            if constexpr (EXT) {
                if (rs.first < 0) rs.first = i + kk;
                mk = (float)(i + kk - rs.first) * delta;
                Wk = opa; Mk = rs.M;
                if constexpr (!BWD) {
                    rs.S1 = rs.S1 + w * (mk * Wk - Mk);
                    rs.S2 = rs.S2 + w * w;
                }
                rs.M = Mk + w * mk;
            }
            img[0] = img[0] + w * col[0]; img[1] = img[1] + w * col[1]; img[2] = img[2] + w * col[2];
            if constexpr (DEPTH) {
                if constexpr (!BWD) rs.Z = rs.Z + w * t;            // the render kernel's dep = dep + w * t
            }
            opa = opa + w;
            T = T * (1.f - alpha);
            if constexpr (BWD) {
                // A_j = sum_c g_c (col_jc - bg); the later samples' share is total minus prefix (the prefix includes sample j)
                float A = 0.f, later = 0.f, dr[3];
                const float rest_o = tt.opa - opa;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if constexpr (RGBA) {
                        A = __builtin_fmaf(tt.g[c], col[c] - tt.b3[c], A);
                        later = __builtin_fmaf(tt.g[c], (tt.img[c] - img[c]) - tt.b3[c] * rest_o, later);
                    } else {
                        A = __builtin_fmaf(tt.g[c], col[c] - tt.bg, A);
                        later = __builtin_fmaf(tt.g[c], (tt.img[c] - img[c]) - tt.bg * rest_o, later);
                    }
                    dr[c] = (raw[c] >= 0.f && raw[c] <= 1.f) ? tt.g[c] * w : 0.f;
                }
                if constexpr (EXT) {
                    // the regularisers are functions of the weights alone: they pass neither clamp.  The photometric share of
                    // `later` above stays what it is (exactly 0 at the last sample); this share carries the rounding of `total`
                    float r = rs.wd * (2.f * (2.f * mk * Wk - 2.f * Mk + rs.mt - mk * tt.opa) + (2.f / 3.f) * delta * w) + rs.re;
                    // the depth term is linear in the weights: its share of A_j is zeta t_j (t carries no gradient)
                    if constexpr (DEPTH) r = r + rs.zeta * t;
                    rs.run = rs.run + w * r;
                    A = A + r;
                    later = later + (rs.total - rs.run);
                }
                const float dsig = delta * (T * A - later);           // T is T_{j+1} here
                if (dsig != 0.f || dr[0] != 0.f || dr[1] != 0.f || dr[2] != 0.f) {     // the same on every lane of the group
#pragma unroll
                    for (int cn = 0; cn < 8; ++cn) {
                        const float tw = ((cn & 4) ? fr[0] : 1.f - fr[0]) * ((cn & 2) ? fr[1] : 1.f - fr[1]) * ((cn & 1) ? fr[2] : 1.f - fr[2]);
                        long long at_row;                                // the corner's row
                        if constexpr (BRICK) {
                            at_row = at[cn];
                            if (at_row < 0) continue;                    // a point of an absent brick has no row: nothing is added
                        } else {
                            at_row = a.slot_of[base + ((cn & 4) ? sx : 0) + ((cn & 2) ? sy : 0) + (cn & 1)];
                            if (at_row < 0 || at_row >= a.n_slots) continue;     // a corner of a support cell always has a slot; never write past the rows
                        }
                        float* row = a.grad + at_row * W;
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

template <int DEG, int G, class Args>
__global__ __launch_bounds__(kBlock) void baked_train_rays_kernel(Args a) {
    constexpr int K = n_coeff(DEG), NCH = rec_bytes(DEG) / 16, CPL = (NCH + G - 1) / G;
    constexpr bool EXT = Args::kExt, RGBA = Args::kRgba, DEPTH = Args::kDepth;
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
    RegState rs{};
    rs.first = -1;
    march<DEG, G, false>(a, o3, d3, near, i0, i1, delta, sub, Y, wr, wg, wb, gy, tt.img, tt.opa, tt, rs);
    tt.bg = a.white ? 1.f : 0.f;
    const float bg = a.white ? 1.f - tt.opa : 0.f;          // the render kernel's expression
    float sq = 0.f;
    bool any = false;
    if constexpr (!EXT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float pre = tt.img[c] + bg, out = fminf(fmaxf(pre, 0.f), 1.f);
            const float diff = out - a.target[ray * 3 + c];
            sq = sq + diff * diff;
            tt.g[c] = (pre >= 0.f && pre <= 1.f) ? diff * a.gscale : 0.f;
            any = any || tt.g[c] != 0.f;
        }
        if (sub == 0 && a.sq_err) a.sq_err[ray] = sq;
    } else {
        const Objective& ob = a.obj;
        float diff[3], dv[3], rv[3];
        bool gate[3];
        [[maybe_unused]] float al = 1.f;                    // RGBA: the ray's alpha; without an alpha array every ray reads 1
        if constexpr (RGBA) {
            // the photograph over the ray's own background: pre = C + b (1 - O) (b = 1: the bits of the white flag's 1 - O; b = 0: of C),
            // tgt = target + (1 - alpha)(b - stored), not clipped
            if (a.rgba.alpha) al = a.rgba.alpha[ray];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                tt.b3[c] = a.rgba.background ? a.rgba.background[ray * 3 + c] : tt.bg;
                const float pre = tt.img[c] + tt.b3[c] * (1.f - tt.opa), out = fminf(fmaxf(pre, 0.f), 1.f);
                float tgt = a.target[ray * 3 + c];
                if (a.rgba.alpha) tgt = tgt + (1.f - al) * (tt.b3[c] - a.rgba.stored);
                diff[c] = out - tgt;
                gate[c] = pre >= 0.f && pre <= 1.f;
                sq = sq + diff[c] * diff[c];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float pre = tt.img[c] + bg, out = fminf(fmaxf(pre, 0.f), 1.f);
                diff[c] = out - a.target[ray * 3 + c];
                gate[c] = pre >= 0.f && pre <= 1.f;
                sq = sq + diff[c] * diff[c];
            }
        }
        // rho and rho' of the ray's three differences: the kind is the same for every ray of the launch, one uniform branch
        if (ob.kind == KNERF_LOSS_MAE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                rv[c] = fabsf(diff[c]);
                dv[c] = diff[c] > 0.f ? 1.f : (diff[c] < 0.f ? -1.f : 0.f);
            }
        } else if (ob.kind == KNERF_LOSS_HUBER) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float ad = fabsf(diff[c]);
                const bool in = ad <= ob.huber_delta;
                rv[c] = in ? 0.5f * (diff[c] * diff[c]) : ob.huber_delta * (ad - 0.5f * ob.huber_delta);
                dv[c] = in ? diff[c] : (diff[c] > 0.f ? ob.huber_delta : -ob.huber_delta);
            }
        } else if (ob.kind == KNERF_LOSS_LOG_COSH) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float ad = fabsf(diff[c]);
                rv[c] = ad + log1pf(expf(-2.f * ad)) - 0.69314718055994531f;
                dv[c] = tanhf(diff[c]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                rv[c] = diff[c] * diff[c];
                dv[c] = 2.f * diff[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            tt.g[c] = gate[c] ? dv[c] * ob.hscale : 0.f;
            any = any || tt.g[c] != 0.f;
        }
        // D, H and what the second march needs of them.  A ray without a fetched sample: D = 0, O = 0, H = H(1e-4)
        const float D = 2.f * rs.S1 + (delta * (1.f / 3.f)) * rs.S2;
        const float O = tt.opa, ac = fminf(fmaxf(O, 1e-4f), 1.f - 1e-4f);
        const float H = -ac * logf(ac) - (1.f - ac) * logf(1.f - ac);
        const float dH = (O >= 1e-4f && O <= 1.f - 1e-4f) ? logf((1.f - ac) / ac) : 0.f;
        // DEPTH: c (Z - z*)^2 and zeta.  A ray of weight 0 has neither, whatever its z* holds (a select: sparse maps are mostly empty)
        [[maybe_unused]] float cz = 1.f, zterm = 0.f;
        if constexpr (DEPTH) {
            if (a.depth.weight) cz = a.depth.weight[ray];
            const float dz = rs.Z - a.depth.target[ray];
            zterm = cz == 0.f ? 0.f : cz * (dz * dz);
            rs.zeta = cz == 0.f ? 0.f : a.depth.wz * (2.f * (cz * dz));
        }
        if (sub == 0) {
            if (a.sq_err) a.sq_err[ray] = sq;
            if (ob.terms) {
                float* tr = ob.terms + ray * (DEPTH ? 6 : RGBA ? 5 : 4);
                tr[0] = (rv[0] + rv[1]) + rv[2]; tr[1] = sq; tr[2] = D; tr[3] = H;
                if constexpr (RGBA) tr[4] = (O - al) * (O - al);
                if constexpr (DEPTH) tr[5] = zterm;
            }
        }
        rs.mt = rs.M; rs.wd = ob.wd; rs.re = ob.we * dH;
        if constexpr (RGBA) {
            // the opacity term (lambda_o / N)(O - alpha)^2 is a function of O alone, as H is: it enters r_j and the total through re
            if (a.rgba.wo > 0.f) rs.re = rs.re + a.rgba.wo * (2.f * (O - al));
        }
        rs.total = ob.wd * (2.f * D) + rs.re * O;
        if constexpr (DEPTH) rs.total = rs.total + rs.zeta * rs.Z;
        rs.M = 0.f; rs.run = 0.f;
        // a ray whose g is 0 on every channel still has the regularisers' gradient once it fetched a sample
        if constexpr (RGBA) any = any || ((ob.wd > 0.f || ob.we > 0.f || a.rgba.wo > 0.f) && rs.first >= 0);
        else any = any || ((ob.wd > 0.f || ob.we > 0.f) && rs.first >= 0);
        // ... and so has the depth term, which passes neither clamp, on a ray whose weight is > 0
        if constexpr (DEPTH) any = any || (cz > 0.f && rs.first >= 0);
    }
    if (!any) return;                                       // the same on every lane of the group
    float img[3], opa;
    march<DEG, G, true>(a, o3, d3, near, i0, i1, delta, sub, Y, wr, wg, wb, gy, img, opa, tt, rs);
}

template <class Args>
hipError_t launch_rays(int deg, int lanes, const Args& a, hipStream_t s) {
    return dispatch_deg_lanes(deg, lanes, [&](auto DEG, auto G) {
        const long long blocks = (a.n * G + kBlock - 1) / kBlock;
        hipLaunchKernelGGL((baked_train_rays_kernel<DEG, G, Args>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
        return hipGetLastError();
    });
}

// the gradient launch of either storage: the plain kernel, or with an objective record the extended one
template <class Args>
hipError_t launch_rays(int deg, int lanes, const Args& a, const Objective* obj, hipStream_t s) {
    if (!obj) return launch_rays(deg, lanes, a, s);
    Ext<Args> e{};
    static_cast<Args&>(e) = a;
    e.obj = *obj;
    return launch_rays(deg, lanes, e, s);
}

// ... or with an rgba record the rgba one (it always carries an objective: that of mean squared error where the caller gave none)
template <class Args>
hipError_t launch_rays(int deg, int lanes, const Args& a, const Objective* obj, const RgbaArgs* rg, hipStream_t s) {
    if (!rg) return launch_rays(deg, lanes, a, obj, s);
    Rgba<Args> e{};
    static_cast<Args&>(e) = a;
    e.obj = *obj;
    e.rgba = *rg;
    return launch_rays(deg, lanes, e, s);
}

// ... or with a depth record the depth one (it always carries an objective and an rgba record: the defaults where the caller gave none)
template <class Args>
hipError_t launch_rays(int deg, int lanes, const Args& a, const Objective* obj, const RgbaArgs* rg, const DepthArgs* dp, hipStream_t s) {
    if (!dp) return launch_rays(deg, lanes, a, obj, rg, s);
    Depth<Args> e{};
    static_cast<Args&>(e) = a;
    e.obj = *obj;
    e.rgba = *rg;
    e.depth = *dp;
    return launch_rays(deg, lanes, e, s);
}

// the objective record of the _ext entry points.  false: KNERF_ERR_INVALID.  plain: NULL, or mse with both weights 0 (the call is then
// the plain launch).  Otherwise `out` is what the extended kernel takes, with the weights and 1 / (3 N) formed in double
static bool check_objective(const knerf_objective* o, uint64_t n_rays, uint64_t n_norm, float* terms, bool& plain, Objective& out) {
    plain = true;
    if (!o) return true;
    if (o->loss_kind < KNERF_LOSS_MSE || o->loss_kind > KNERF_LOSS_LOG_COSH) return false;
    if (o->loss_kind == KNERF_LOSS_HUBER && (!(o->huber_delta > 0.f) || !std::isfinite(o->huber_delta))) return false;
    if (!(o->distortion >= 0.f) || !std::isfinite(o->distortion)) return false;
    if (!(o->opacity_entropy >= 0.f) || !std::isfinite(o->opacity_entropy)) return false;
    plain = o->loss_kind == KNERF_LOSS_MSE && o->distortion == 0.f && o->opacity_entropy == 0.f;
    const double N = (double)(n_norm ? n_norm : (n_rays ? n_rays : 1));
    out.kind = o->loss_kind;
    out.huber_delta = o->loss_kind == KNERF_LOSS_HUBER ? o->huber_delta : 0.f;
    out.hscale = (float)(1.0 / (3.0 * N));
    out.wd = (float)((double)o->distortion / N);
    out.we = (float)((double)o->opacity_entropy / N);
    out.terms = terms;
    return true;
}

// the rgba record of the _rgba entry points.  false: KNERF_ERR_INVALID.  none: NULL, or no background, no alpha and weight 0 (the call is
// then the _ext call).  Otherwise `out` is what the rgba kernel takes and `obj` is filled even for the plain objective (the rgba kernel
// is an extended one: it evaluates mean squared error as the objective's kind 0)
static bool check_rgba(const knerf_baked_rgba* r, const knerf_objective* objective, uint64_t n_rays, uint64_t n_norm, float* terms,
                       bool& none, RgbaArgs& out, Objective& obj) {
    none = true;
    if (!r) return true;
    if (!(r->stored_background == 0.f || r->stored_background == 1.f)) return false;
    if (!(r->opacity >= 0.f) || !std::isfinite(r->opacity)) return false;
    if (r->opacity > 0.f && !r->alpha) return false;
    none = !r->background && !r->alpha && r->opacity == 0.f;
    if (none) return true;
    const double N = (double)(n_norm ? n_norm : (n_rays ? n_rays : 1));
    out.background = r->background; out.alpha = r->alpha; out.stored = r->stored_background;
    out.wo = (float)((double)r->opacity / N);
    if (!objective) {
        knerf_objective mse{};
        mse.loss_kind = KNERF_LOSS_MSE;
        bool plain = true;
        return check_objective(&mse, n_rays, n_norm, terms, plain, obj);
    }
    return true;
}

// the depth record of the _depth entry points.  false: KNERF_ERR_INVALID.  off: NULL or weight 0 (the call is then the _rgba call).
// Otherwise `out` is what the depth kernel takes, `obj` is filled even for the plain objective and `rg` holds the rgba contract's
// defaults where there is no rgba record (no background but the flag's, every alpha 1, no opacity loss)
static bool check_depth(const knerf_baked_depth* z, const knerf_objective* objective, bool none, uint64_t n_rays, uint64_t n_norm,
                        float* terms, bool& off, DepthArgs& out, RgbaArgs& rg, Objective& obj) {
    off = true;
    if (!z) return true;
    if (!(z->depth >= 0.f) || !std::isfinite(z->depth)) return false;
    if (z->depth > 0.f && !z->target) return false;
    off = z->depth == 0.f;
    if (off) return true;
    const double N = (double)(n_norm ? n_norm : (n_rays ? n_rays : 1));
    out.target = z->target; out.weight = z->weight;
    out.wz = (float)((double)z->depth / N);
    if (none) rg = RgbaArgs{};
    if (!objective && none) {
        knerf_objective mse{};
        mse.loss_kind = KNERF_LOSS_MSE;
        bool plain = true;
        return check_objective(&mse, n_rays, n_norm, terms, plain, obj);
    }
    return true;
}

struct ApplyArgs {
    uint4* rec;
    const int* point_of;
    const unsigned char* trainable;
    float *w, *m, *v, *g;
    long long n_slots, n_points;
    int K, nch;
    float rate_sigma, rate_sh, b1, b2, eps;
};

__global__ __launch_bounds__(256) void baked_train_apply_kernel(ApplyArgs a) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n_slots * a.nch) return;
    const long long slot = idx / a.nch;
    const int q = (int)(idx - slot * a.nch);
    const long long row = slot * (1 + 3 * a.K);
    float sig = 0.f;
    if (q == 0) {
        sig = fmaxf(adam(a, row, a.rate_sigma, a.trainable[slot] != 0), 0.f);      // the projection; an untrainable sigma is and stays 0
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
    const long long p = a.point_of[slot];
    if (p < 0 || p >= a.n_points) return;
    uint4 out;
    out.x = q == 0 ? __float_as_uint(sig) : (h[0] | (h[1] << 16));
    out.y = h[2] | (h[3] << 16);
    out.z = h[4] | (h[5] << 16);
    out.w = h[6] | (h[7] << 16);
    a.rec[p * a.nch + q] = out;
}

struct BrickApplyArgs {
    uint4* rec;
    const unsigned char* flags;
    float *w, *m, *v, *g;
    long long n_records;
    int K, nch;
    float rate_sigma, rate_sh, b1, b2, eps;
};

__global__ __launch_bounds__(256) void baked_bricks_train_apply_kernel(BrickApplyArgs a) {
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

// what every entry point of the dense optimiser checks of its struct; the lattice's points come back
static bool check_state(const knerf_baked_train* t, unsigned long long& points) {
    if (!t || !t->field.records || !t->field.bits || !t->slot_of || !t->grad) return false;
    if (!check_lattice(t->field.resolution, t->field.lo, t->field.hi, t->field.sh_degree, nullptr, points)) return false;
    // a slot is a lattice point: at least one, at most all of them (the rows then stay below 2^40 bytes with the records)
    return t->n_slots >= 1 && t->n_slots <= points;
}

// the same for the brick optimiser: what knerf_baked_render_bricks refuses of its struct, and the NULLs this one adds
static bool check_state(const knerf_baked_bricks_train* t, int (&B)[3], float (&scale)[3], unsigned long long& n_records) {
    if (!t || !t->field.records || !t->field.brick_of || !t->field.bits || !t->grad) return false;
    const knerf_baked_bricks* f = &t->field;
    unsigned long long points = 0;
    if (!check_lattice(f->resolution, f->lo, f->hi, f->sh_degree, scale, points)) return false;
    if (!check_brick_grid(f->resolution, f->sh_degree, f->brick_log2, f->n_bricks, B)) return false;
    n_records = f->n_bricks << (3 * f->brick_log2);
    return true;
}

// the ray arguments of both gradient launches; lanes comes back resolved.  n_rays = 0 is for the caller
static bool check_train_rays(int deg, const float* origins, const float* directions, const float* near, const float* far, float near_all,
                             float far_all, const float* target, uint64_t n_rays, uint64_t n_norm, float step, float termination,
                             int flags, int& lanes) {
    if (!origins || !directions || !target) return false;
    if (!check_rays(near, far, near_all, far_all, n_rays, step, termination, flags) || n_norm >= (1ull << 36)) return false;
    lanes = pick_lanes(deg, flags, kLaneGroups);
    return lanes != 0;
}

// the same fields in both argument structs
template <class Args>
static void set_rays(Args& a, const float* origins, const float* directions, const float* near, const float* far, float near_all,
                     float far_all, const float* target, uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags,
                     float* grad, float* sq_err) {
    a.o = origins; a.d = directions; a.near = near; a.far = far; a.near0 = near_all; a.far0 = far_all; a.target = target;
    a.n = (long long)n_rays; a.step = step; a.eps = termination;
    a.gscale = (float)(2.0 / (3.0 * (double)(n_norm ? n_norm : n_rays)));
    a.white = (flags & KNERF_BAKED_WHITE_BACKGROUND) ? 1 : 0;
    a.grad = grad; a.sq_err = sq_err;
}

static bool check_adam(float rate_sigma, float rate_sh, float beta_1, float beta_2, float epsilon) {
    return std::isfinite(rate_sigma) && std::isfinite(rate_sh) && (beta_1 >= 0.f && beta_1 < 1.f) && (beta_2 >= 0.f && beta_2 < 1.f) &&
           (epsilon > 0.f) && std::isfinite(epsilon);
}

}  // namespace baked_train
}  // namespace knerf

using namespace knerf;

// knerf_baked_train_rays (objective = NULL), knerf_baked_train_rays_ext (rgba = NULL) and knerf_baked_train_rays_rgba
static int train_rays(void* stream, const knerf_baked_train* train, const float* origins, const float* directions, const float* near,
                      const float* far, float near_all, float far_all, const float* target, uint64_t n_rays, uint64_t n_norm, float step,
                      float termination, int flags, float* sq_err, const knerf_objective* objective, float* terms,
                      const knerf_baked_rgba* rgba = nullptr, const knerf_baked_depth* depth = nullptr) {
    unsigned long long points = 0;
    int lanes = 0;
    bool plain = true, none = true, off = true;
    baked_train::Objective obj{};
    baked_train::RgbaArgs rg{};
    baked_train::DepthArgs dp{};
    if (!baked_train::check_state(train, points)) return KNERF_ERR_INVALID;
    if (!baked_train::check_objective(objective, n_rays, n_norm, terms, plain, obj)) return KNERF_ERR_INVALID;
    if (!baked_train::check_rgba(rgba, objective, n_rays, n_norm, terms, none, rg, obj)) return KNERF_ERR_INVALID;
    if (!baked_train::check_depth(depth, objective, none, n_rays, n_norm, terms, off, dp, rg, obj)) return KNERF_ERR_INVALID;
    const knerf_baked_field* field = &train->field;
    const int deg = field->sh_degree;
    if (!baked_train::check_train_rays(deg, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination,
                                       flags, lanes))
        return KNERF_ERR_INVALID;
    baked_train::TrainArgs a{};
    if (!baked::check_lattice(field->resolution, field->lo, field->hi, deg, a.scale, points)) return KNERF_ERR_INVALID;
    if (n_rays == 0) return KNERF_OK;
    for (int c = 0; c < 3; ++c) { a.R[c] = field->resolution[c]; a.lo[c] = field->lo[c]; a.hi[c] = field->hi[c]; }
    a.rec = static_cast<const uint4*>(field->records); a.bits = field->bits;
    a.slot_of = train->slot_of; a.n_slots = (long long)train->n_slots;
    baked_train::set_rays(a, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination, flags,
                          train->grad, sq_err);
    return baked_train::launch_rays(deg, lanes, a, plain && none && off ? nullptr : &obj, none && off ? nullptr : &rg, off ? nullptr : &dp,
                                    (hipStream_t)stream) == hipSuccess
               ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_train_rays_rgba(void* stream, const knerf_baked_train* train, const float* origins, const float* directions,
                                           const float* near, const float* far, float near_all, float far_all, const float* target,
                                           uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* sq_err,
                                           const knerf_objective* objective, float* terms, const knerf_baked_rgba* rgba) {
    return train_rays(stream, train, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination, flags,
                      sq_err, objective, terms, rgba);
}

extern "C" int knerf_baked_train_rays_depth(void* stream, const knerf_baked_train* train, const float* origins, const float* directions,
                                            const float* near, const float* far, float near_all, float far_all, const float* target,
                                            uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* sq_err,
                                            const knerf_objective* objective, float* terms, const knerf_baked_rgba* rgba,
                                            const knerf_baked_depth* depth) {
    return train_rays(stream, train, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination, flags,
                      sq_err, objective, terms, rgba, depth);
}

extern "C" int knerf_baked_train_rays(void* stream, const knerf_baked_train* train, const float* origins, const float* directions,
                                      const float* near, const float* far, float near_all, float far_all, const float* target,
                                      uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* sq_err) {
    return train_rays(stream, train, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination, flags,
                      sq_err, nullptr, nullptr);
}

extern "C" int knerf_baked_train_rays_ext(void* stream, const knerf_baked_train* train, const float* origins, const float* directions,
                                          const float* near, const float* far, float near_all, float far_all, const float* target,
                                          uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags, float* sq_err,
                                          const knerf_objective* objective, float* terms) {
    return train_rays(stream, train, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination, flags,
                      sq_err, objective, terms);
}

extern "C" int knerf_baked_train_apply(void* stream, const knerf_baked_train* train, const int32_t* point_of,
                                       const uint8_t* sigma_trainable, float* master, float* m, float* v, float rate_sigma, float rate_sh,
                                       float beta_1, float beta_2, float epsilon) {
    unsigned long long points = 0;
    if (!baked_train::check_state(train, points) || !point_of || !sigma_trainable || !master || !m || !v) return KNERF_ERR_INVALID;
    if (!baked_train::check_adam(rate_sigma, rate_sh, beta_1, beta_2, epsilon)) return KNERF_ERR_INVALID;
    const int deg = train->field.sh_degree;
    baked_train::ApplyArgs a{};
    a.rec = static_cast<uint4*>(const_cast<void*>(train->field.records));
    a.point_of = point_of; a.trainable = sigma_trainable; a.w = master; a.m = m; a.v = v; a.g = train->grad;
    a.n_slots = (long long)train->n_slots; a.n_points = (long long)points;
    a.K = baked::n_coeff(deg); a.nch = baked::rec_bytes(deg) / 16;
    a.rate_sigma = rate_sigma; a.rate_sh = rate_sh; a.b1 = beta_1; a.b2 = beta_2; a.eps = epsilon;
    const unsigned long long blocks = (train->n_slots * (unsigned)a.nch + 255) / 256;
    if (blocks >= (1ull << 31)) return KNERF_ERR_INVALID;
    hipLaunchKernelGGL(baked_train::baked_train_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

// knerf_baked_bricks_train_rays (objective = NULL) and knerf_baked_bricks_train_rays_ext
static int bricks_train_rays(void* stream, const knerf_baked_bricks_train* train, const float* origins, const float* directions,
                             const float* near, const float* far, float near_all, float far_all, const float* target, uint64_t n_rays,
                             uint64_t n_norm, float step, float termination, int flags, float* sq_err, const knerf_objective* objective,
                             float* terms, const knerf_baked_rgba* rgba = nullptr, const knerf_baked_depth* depth = nullptr) {
    int B[3], lanes = 0;
    unsigned long long n_records = 0;
    bool plain = true, none = true, off = true;
    baked_train::Objective obj{};
    baked_train::RgbaArgs rg{};
    baked_train::DepthArgs dp{};
    baked_train::BrickTrainArgs a{};
    if (!baked_train::check_state(train, B, a.scale, n_records)) return KNERF_ERR_INVALID;
    if (!baked_train::check_objective(objective, n_rays, n_norm, terms, plain, obj)) return KNERF_ERR_INVALID;
    if (!baked_train::check_rgba(rgba, objective, n_rays, n_norm, terms, none, rg, obj)) return KNERF_ERR_INVALID;
    if (!baked_train::check_depth(depth, objective, none, n_rays, n_norm, terms, off, dp, rg, obj)) return KNERF_ERR_INVALID;
    const knerf_baked_bricks* field = &train->field;
    const int deg = field->sh_degree;
    // every lane variant of knerf_baked_train_rays exists here too: each builds without scratch (DESIGN.md 2.23 has hipcc's counts)
    if (!baked_train::check_train_rays(deg, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination,
                                       flags, lanes))
        return KNERF_ERR_INVALID;
    if (n_rays == 0) return KNERF_OK;
    for (int c = 0; c < 3; ++c) { a.R[c] = field->resolution[c]; a.lo[c] = field->lo[c]; a.hi[c] = field->hi[c]; }
    a.rec = static_cast<const uint4*>(field->records); a.brick_of = field->brick_of; a.bits = field->bits;
    a.L = field->brick_log2; a.By = B[1]; a.Bz = B[2]; a.n_bricks = (long long)field->n_bricks;
    baked_train::set_rays(a, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination, flags,
                          train->grad, sq_err);
    return baked_train::launch_rays(deg, lanes, a, plain && none && off ? nullptr : &obj, none && off ? nullptr : &rg, off ? nullptr : &dp,
                                    (hipStream_t)stream) == hipSuccess
               ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_bricks_train_rays_rgba(void* stream, const knerf_baked_bricks_train* train, const float* origins,
                                                  const float* directions, const float* near, const float* far, float near_all,
                                                  float far_all, const float* target, uint64_t n_rays, uint64_t n_norm, float step,
                                                  float termination, int flags, float* sq_err, const knerf_objective* objective,
                                                  float* terms, const knerf_baked_rgba* rgba) {
    return bricks_train_rays(stream, train, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination,
                             flags, sq_err, objective, terms, rgba);
}

extern "C" int knerf_baked_bricks_train_rays_depth(void* stream, const knerf_baked_bricks_train* train, const float* origins,
                                                   const float* directions, const float* near, const float* far, float near_all,
                                                   float far_all, const float* target, uint64_t n_rays, uint64_t n_norm, float step,
                                                   float termination, int flags, float* sq_err, const knerf_objective* objective,
                                                   float* terms, const knerf_baked_rgba* rgba, const knerf_baked_depth* depth) {
    return bricks_train_rays(stream, train, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination,
                             flags, sq_err, objective, terms, rgba, depth);
}

extern "C" int knerf_baked_bricks_train_rays(void* stream, const knerf_baked_bricks_train* train, const float* origins,
                                             const float* directions, const float* near, const float* far, float near_all, float far_all,
                                             const float* target, uint64_t n_rays, uint64_t n_norm, float step, float termination, int flags,
                                             float* sq_err) {
    return bricks_train_rays(stream, train, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination,
                             flags, sq_err, nullptr, nullptr);
}

extern "C" int knerf_baked_bricks_train_rays_ext(void* stream, const knerf_baked_bricks_train* train, const float* origins,
                                                 const float* directions, const float* near, const float* far, float near_all,
                                                 float far_all, const float* target, uint64_t n_rays, uint64_t n_norm, float step,
                                                 float termination, int flags, float* sq_err, const knerf_objective* objective,
                                                 float* terms) {
    return bricks_train_rays(stream, train, origins, directions, near, far, near_all, far_all, target, n_rays, n_norm, step, termination,
                             flags, sq_err, objective, terms);
}

extern "C" int knerf_baked_bricks_train_apply(void* stream, const knerf_baked_bricks_train* train, const uint8_t* flags, float* master,
                                              float* m, float* v, float rate_sigma, float rate_sh, float beta_1, float beta_2,
                                              float epsilon) {
    int B[3];
    float scale[3];
    unsigned long long n_records = 0;
    if (!baked_train::check_state(train, B, scale, n_records) || !flags || !master || !m || !v) return KNERF_ERR_INVALID;
    if (!baked_train::check_adam(rate_sigma, rate_sh, beta_1, beta_2, epsilon)) return KNERF_ERR_INVALID;
    const int deg = train->field.sh_degree;
    baked_train::BrickApplyArgs a{};
    a.rec = static_cast<uint4*>(const_cast<void*>(train->field.records));
    a.flags = flags; a.w = master; a.m = m; a.v = v; a.g = train->grad;
    a.n_records = (long long)n_records;
    a.K = baked::n_coeff(deg); a.nch = baked::rec_bytes(deg) / 16;
    a.rate_sigma = rate_sigma; a.rate_sh = rate_sh; a.b1 = beta_1; a.b2 = beta_2; a.eps = epsilon;
    const unsigned long long blocks = (n_records * (unsigned)a.nch + 255) / 256;
    if (blocks >= (1ull << 31)) return KNERF_ERR_INVALID;
    hipLaunchKernelGGL(baked_train::baked_bricks_train_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
