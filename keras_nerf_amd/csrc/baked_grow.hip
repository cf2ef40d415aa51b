// baked_grow.hip -- what turns the fine-tuner of baked_train.hip into a grid trainer (gfx950), context-free: a total-variation
// regulariser over the slots of an optimiser and the resampling of a field onto another lattice (coarse to fine).  Extension: the
// reference has nothing of the kind (Plenoxels and its kin regularise and refine their grids in this way).  include/knerf.h holds
// the contract; tests/baked_grow_reference.py is its NumPy restatement.  The record's sizes and codec and the lattice check are those
// of baked_common.h; the arithmetic of a point is that of baked_grow_common.h, which baked_bricks_grow.hip shares.
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
#include "baked_grow_common.h"

namespace knerf {
namespace baked_grow {

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
            const int z = (int)(p % a.R[2]);
            const long long xy = p / a.R[2];
            const int y = (int)(xy % a.R[1]), x = (int)(xy / a.R[1]);
            tv0 = tv_column<W>(a.master, a.grad, a.eps, w, slot, q,
                               [&](int dx, int dy, int dz) { return slot_at(a, x + dx, y + dy, z + dz); });
        }
    }
    if (a.tv_out) tv_store<W>(terms, t, valid && q == 0, tv0, a.tv_out, slot);      // the same for every lane of the launch
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
    uint4 old[8];                                        // the chunk of the 8 surrounding old records
#pragma unroll
    for (int cn = 0; cn < 8; ++cn) {
        const long long pt = ((long long)(cx + (cn >> 2)) * a.R[1] + (cy + ((cn >> 1) & 1))) * a.R[2] + (cz + (cn & 1));
        old[cn] = a.src[pt * a.nch + qc];
    }
    a.dst[idx] = resample_chunk(old, qc, a.K, fx, fy, fz, a.threshold);
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
    if (!baked_grow::check_tv(weight_sigma, weight_sh, epsilon)) return KNERF_ERR_INVALID;
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
