// baked_common.h -- what every baked-field kernel file (baked*.hip) shares, defined once: the record's sizes and its fp16 codec, the SH
// basis, the DPP group sums, locate, the Adam column, and the host-side argument checks of the entry points.  Each kernel keeps its own
// argument struct; locate and adam are templates on it and read the fields by name (a.lo, a.scale, a.R, a.step; a.g, a.w, a.m, a.v,
// a.b1, a.b2, a.eps), so no kernel's argument layout depends on this file.
// What is NOT here although every march has it: the per-lane basis tables, the sample range, a batch's occupancy mask and the 8 corner
// addresses of a brick field.  They have loops, branches or arrays, and hipcc compiles them differently when they come into a kernel
// through a function (it simplifies each function on its own before it inlines): different instruction counts in every kernel that
// was tried.  Straight-line helpers such as the ones here come out instruction for instruction as the text in place did.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/knerf.h"

namespace knerf {
namespace baked {

constexpr int kBlock = 256;
constexpr int kBatch = 8;                           // samples whose occupancy bits are looked up together
constexpr int kMaxSamples = 1 << 23;               // (float)i + 0.5f is exact below this
constexpr unsigned long long kMaxBytes = 1ull << 40;

__host__ __device__ constexpr int n_coeff(int deg) { return (deg + 1) * (deg + 1); }
__host__ __device__ constexpr int rec_bytes(int deg) { return (4 + 6 * n_coeff(deg) + 15) / 16 * 16; }

__device__ __forceinline__ float half_bits_to_float(unsigned h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(h & 0xffffu)); }
__device__ __forceinline__ unsigned float_to_half_bits(float f) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)f); }   // round to nearest even

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

// Keras-form Adam on one column of the rows (a.g, a.w, a.m, a.v; a.b1, a.b2, a.eps): the gradient is taken and zeroed, the new master
// value comes back (the old one where the column does not train)
template <class Args>
__device__ __forceinline__ float adam(const Args& a, long long at, float rate, bool train) {
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

// sample i of a ray: t_i, and if the sample lies inside the box (the return value) its cell and the trilinear fractions
template <class Args>
__device__ __forceinline__ bool locate(const Args& a, float near, const float (&o3)[3], const float (&d3)[3], int i, float& t,
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

// log2 of the brick edge of an argument struct (Args::kBrick, a.L); 0 for dense storage, which has none
template <class Args>
__device__ __forceinline__ int brick_log2(const Args& a) {
    if constexpr (Args::kBrick) return a.L; else return 0;
}

// ---- the entry points' argument checks (host).  Each returns false for what its entry points answer with KNERF_ERR_INVALID

// a lattice knerf_baked_render takes: degree, resolution, box, table size; its points in `points`.  scale: cells / (hi - lo) per axis as
// locate wants it, refused where it is not finite in fp32; nullptr where the caller marches no ray (then it is not formed)
inline bool check_lattice(const int32_t* resolution, const float* lo, const float* hi, int deg, float* scale, unsigned long long& points) {
    if (deg < 0 || deg > 3) return false;
    points = 1;
    for (int c = 0; c < 3; ++c) {
        const int r = resolution[c];
        if (r < 2 || r > 1025) return false;
        if (!std::isfinite(lo[c]) || !std::isfinite(hi[c]) || !(hi[c] > lo[c])) return false;
        if (scale) {
            scale[c] = (float)((double)(r - 1) / ((double)hi[c] - (double)lo[c]));
            if (!std::isfinite(scale[c])) return false;
        }
        points *= (unsigned)r;
    }
    return points < kMaxBytes / (unsigned)rec_bytes(deg);
}

// the brick set over a lattice check_lattice has passed: the brick edge, the brick grid B, the number of stored bricks and their bytes
inline bool check_brick_grid(const int32_t* resolution, int deg, int brick_log2, unsigned long long n_bricks, int (&B)[3]) {
    const int L = brick_log2;
    if (L != 2 && L != 3) return false;
    unsigned long long grid = 1;
    for (int c = 0; c < 3; ++c) {
        B[c] = (resolution[c] + (1 << L) - 1) >> L;
        grid *= (unsigned)B[c];
    }
    if (n_bricks == 0 || n_bricks > grid) return false;
    return (n_bricks << (3 * L)) < kMaxBytes / (unsigned)rec_bytes(deg);
}

// the ray arguments every march takes
inline bool check_rays(const float* near, const float* far, float near_all, float far_all, uint64_t n_rays, float step, float termination,
                       int flags) {
    if (flags & ~(KNERF_BAKED_WHITE_BACKGROUND | KNERF_BAKED_SKIP_EMPTY | KNERF_BAKED_LANES_MASK)) return false;
    if (!(step > 0.f) || !std::isfinite(step) || !(termination >= 0.f) || !(termination < 1.f)) return false;
    if ((!near && !std::isfinite(near_all)) || (!far && !std::isfinite(far_all))) return false;
    return n_rays < (1ull << 36);
}

// lanes per ray: what the flags ask for, or group[deg] where they leave the choice to the library.  A degree has the one-lane variant
// and the group variant group[deg]; 0 comes back for any other count
constexpr int kLaneGroups[4] = {1, 2, 4, 4};
inline int pick_lanes(int deg, int flags, const int (&group)[4]) {
    int lanes = (flags & KNERF_BAKED_LANES_MASK) >> KNERF_BAKED_LANES_SHIFT;
    if (lanes == 0) lanes = group[deg];
    return (lanes == 1 || lanes == group[deg]) ? lanes : 0;
}

// f(std::integral_constant<int, DEG>, std::integral_constant<int, G>) for the lane variants of kLaneGroups
template <class F>
hipError_t dispatch_deg_lanes(int deg, int lanes, F&& f) {
    using std::integral_constant;
    switch (deg * 8 + lanes) {
        case 0 * 8 + 1: return f(integral_constant<int, 0>{}, integral_constant<int, 1>{});
        case 1 * 8 + 1: return f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
        case 1 * 8 + 2: return f(integral_constant<int, 1>{}, integral_constant<int, 2>{});
        case 2 * 8 + 1: return f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
        case 2 * 8 + 4: return f(integral_constant<int, 2>{}, integral_constant<int, 4>{});
        case 3 * 8 + 1: return f(integral_constant<int, 3>{}, integral_constant<int, 1>{});
        case 3 * 8 + 4: return f(integral_constant<int, 3>{}, integral_constant<int, 4>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace baked
}  // namespace knerf
