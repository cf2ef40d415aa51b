// baked_bricks_grow.hip -- growing a baked field on its brick storage (gfx950), context-free: baked_grow.hip's resampling and
// total-variation regulariser with a lattice point's record or row found through the brick table, so that a field is refined, regularised
// and pruned without the dense record table ever existing.  Extension: the reference has nothing of the kind.  include/knerf.h holds the
// contract; tests/baked_bricks_grow_reference.py is its NumPy restatement.  The arithmetic of a point is baked_grow_common.h's, the text
// baked_grow.hip uses: the results are the dense kernels' bit for bit.
//
//   baked_bricks_sigma_kernel     one lane per new lattice point: sigma of the 8 surrounding old points (4 bytes each, through the source's
//                                 brick table), trilinear, thresholded.  The caller builds the new occupancy bits and brick table from it.
//   baked_bricks_resample_kernel  one lane per (destination record, 16-byte chunk), as baked_resample_kernel.  A record knows its brick from
//                                 dst_keys and its place from its index; a place past the lattice or a key outside the brick grid is
//                                 written as zeros.
//   baked_bricks_tv_kernel <W>    baked_tv_kernel's shape: one lane per (stored record, column), floor(256 / W) whole rows per block, tv_out
//                                 summed in LDS.  A neighbour inside the lane's own brick is the row +-1, +-b, +-b^2 (its place is formed
//                                 from the coordinates, which is the same number); one across a brick face goes through brick_of behind a
//                                 one-entry cache.  A neighbour takes part iff its flag has bit 0.
// Every lookup is checked before an address is formed: a point outside the lattice is never looked up, a brick_of value < 0 or >= n_bricks
// is an absent brick, a key outside the brick grid makes its records inert.  Record and row offsets are 64-bit.
#include "baked_common.h"
#include "baked_grow_common.h"

namespace knerf {
namespace baked_bricks_grow {
using namespace baked;
using namespace baked_grow;

// a brick set as the kernels read it
struct Bricks {
    const uint4* rec;
    const int* brick_of;
    long long n_bricks;
    int R[3];
    int L, By, Bz, nch;
};

// the place of lattice point (x, y, z) inside its brick
__device__ __forceinline__ int place_in(int L, int x, int y, int z) {
    const int inm = (1 << L) - 1;
    return ((((x & inm) << L) | (y & inm)) << L) | (z & inm);
}

// the stored brick of the brick grid's entry `key` behind a one-entry cache, -1 for an absent one (or a value the set does not have)
__device__ __forceinline__ long long brick_at(const int* brick_of, long long n_bricks, int key, int& last_key, int& last_slot) {
    const int slot = key == last_key ? last_slot : brick_of[key];
    last_key = key; last_slot = slot;
    return (slot >= 0 && (long long)slot < n_bricks) ? (long long)slot : -1;
}

// the record index of lattice point (x, y, z), which the caller knows to lie in the lattice; -1 in an absent brick
__device__ __forceinline__ long long record_at(const Bricks& f, int x, int y, int z, int& last_key, int& last_slot) {
    const int key = ((x >> f.L) * f.By + (y >> f.L)) * f.Bz + (z >> f.L);
    const long long slot = brick_at(f.brick_of, f.n_bricks, key, last_key, last_slot);
    return slot < 0 ? -1 : ((slot << (3 * f.L)) | (long long)place_in(f.L, x, y, z));
}

struct SigmaArgs {
    Bricks src;
    float* dst;
    int Rn[3];
    long long n_new;
    float threshold;
};

__global__ __launch_bounds__(kBlock) void baked_bricks_sigma_kernel(SigmaArgs a) {
    const long long pn = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (pn >= a.n_new) return;
    const int k = (int)(pn % a.Rn[2]);
    const long long ij = pn / a.Rn[2];
    const int j = (int)(ij % a.Rn[1]), i = (int)(ij / a.Rn[1]);
    int cx, cy, cz;
    float fx, fy, fz;
    place(i, a.src.R[0], a.Rn[0], cx, fx);
    place(j, a.src.R[1], a.Rn[1], cy, fy);
    place(k, a.src.R[2], a.Rn[2], cz, fz);
    const unsigned* words = reinterpret_cast<const unsigned*>(a.src.rec);
    int last_key = -1, last_slot = -1;
    unsigned first[8];
#pragma unroll
    for (int cn = 0; cn < 8; ++cn) {
        const long long r = record_at(a.src, cx + (cn >> 2), cy + ((cn >> 1) & 1), cz + (cn & 1), last_key, last_slot);
        first[cn] = r >= 0 ? words[r * a.src.nch * 4] : 0u;
    }
    a.dst[pn] = resample_sigma(first, fx, fy, fz, a.threshold);
}

struct ResampleArgs {
    Bricks src;
    uint4* dst;
    const int* keys;
    long long n_records, grid;          // destination records; entries of the destination's brick grid
    int Rn[3];
    int L, By, Bz, K;                   // the destination's brick edge and grid
    float threshold;
};

__global__ __launch_bounds__(kBlock) void baked_bricks_resample_kernel(ResampleArgs a) {
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= a.n_records * a.src.nch) return;
    const long long record = idx / a.src.nch;
    const int qc = (int)(idx - record * a.src.nch);
    const int in = (int)(record & ((1ll << (3 * a.L)) - 1)), inm = (1 << a.L) - 1;
    const long long key = a.keys[record >> (3 * a.L)];
    uint4 out = make_uint4(0u, 0u, 0u, 0u);
    if (key >= 0 && key < a.grid) {
        const int bz = (int)(key % a.Bz);
        const long long bxy = key / a.Bz;
        const int by = (int)(bxy % a.By), bx = (int)(bxy / a.By);
        const int i = (bx << a.L) | (in >> (2 * a.L)), j = (by << a.L) | ((in >> a.L) & inm), k = (bz << a.L) | (in & inm);
        if (i < a.Rn[0] && j < a.Rn[1] && k < a.Rn[2]) {
            int cx, cy, cz;
            float fx, fy, fz;
            place(i, a.src.R[0], a.Rn[0], cx, fx);
            place(j, a.src.R[1], a.Rn[1], cy, fy);
            place(k, a.src.R[2], a.Rn[2], cz, fz);
            int last_key = -1, last_slot = -1;
            uint4 old[8];
#pragma unroll
            for (int cn = 0; cn < 8; ++cn) {
                const long long r = record_at(a.src, cx + (cn >> 2), cy + ((cn >> 1) & 1), cz + (cn & 1), last_key, last_slot);
                old[cn] = r >= 0 ? a.src.rec[r * a.src.nch + qc] : make_uint4(0u, 0u, 0u, 0u);
            }
            out = resample_chunk(old, qc, a.K, fx, fy, fz, a.threshold);
        }
    }
    a.dst[idx] = out;
}

struct TvArgs {
    const int* brick_of;
    const int* keys;
    const unsigned char* flags;
    const float* master;
    float* grad;
    float* tv_out;
    long long n_bricks, n_records, grid;
    int R[3];
    int L, By, Bz;
    float w_sigma, w_sh, eps;
};

template <int W>
__global__ __launch_bounds__(kBlock) void baked_bricks_tv_kernel(TvArgs a) {
    constexpr int S = kBlock / W;                        // whole rows per block
    __shared__ float terms[kBlock];
    const int t = threadIdx.x;
    const int ls = t / W, q = t - ls * W;
    const long long record = (long long)blockIdx.x * S + ls;
    const bool valid = ls < S && record < a.n_records;
    const float w = q == 0 ? a.w_sigma : a.w_sh;
    float tv0 = 0.f;
    if (valid && (w != 0.f || a.tv_out) && (a.flags[record] & 1u)) {
        const int L = a.L, inm = (1 << L) - 1;
        const long long slot = record >> (3 * L), key = a.keys[slot];
        const int in = (int)(record & ((1ll << (3 * L)) - 1));
        if (key >= 0 && key < a.grid) {
            const int bz = (int)(key % a.Bz);
            const long long bxy = key / a.Bz;
            const int by = (int)(bxy % a.By), bx = (int)(bxy / a.By);
            const int x = (bx << L) | (in >> (2 * L)), y = (by << L) | ((in >> L) & inm), z = (bz << L) | (in & inm);
            if (x < a.R[0] && y < a.R[1] && z < a.R[2]) {
                int last_key = -1, last_slot = -1;
                // the row of the point at an offset from this one: in the lattice, in a stored brick, a slot
                auto row_at = [&](int dx, int dy, int dz) -> long long {
                    const int X = x + dx, Y = y + dy, Z = z + dz;
                    if (X < 0 || Y < 0 || Z < 0 || X >= a.R[0] || Y >= a.R[1] || Z >= a.R[2]) return -1;
                    long long brick = slot;
                    if ((X >> L) != bx || (Y >> L) != by || (Z >> L) != bz) {            // across a brick face
                        brick = brick_at(a.brick_of, a.n_bricks, ((X >> L) * a.By + (Y >> L)) * a.Bz + (Z >> L), last_key, last_slot);
                        if (brick < 0) return -1;
                    }
                    const long long r = (brick << (3 * L)) | (long long)place_in(L, X, Y, Z);
                    return (a.flags[r] & 1u) ? r : -1;
                };
                tv0 = tv_column<W>(a.master, a.grad, a.eps, w, record, q, row_at);
            }
        }
    }
    if (a.tv_out) tv_store<W>(terms, t, valid && q == 0, tv0, a.tv_out, record);     // the same for every lane of the launch
}

template <int W>
hipError_t launch_tv(const TvArgs& a, hipStream_t s) {
    constexpr int S = kBlock / W;
    const long long blocks = (a.n_records + S - 1) / S;
    if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((baked_bricks_tv_kernel<W>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// what knerf_baked_render_bricks refuses of its field; the brick grid comes back.  records: whether the set's own records are read
static bool check_bricks(const knerf_baked_bricks* f, bool records, int (&B)[3]) {
    if (!f || (records && !f->records) || !f->brick_of) return false;
    unsigned long long points = 0;
    float scale[3];
    if (!check_lattice(f->resolution, f->lo, f->hi, f->sh_degree, scale, points)) return false;
    return check_brick_grid(f->resolution, f->sh_degree, f->brick_log2, f->n_bricks, B);
}

static void set_bricks(Bricks& b, const knerf_baked_bricks* f, const int (&B)[3]) {
    b.rec = static_cast<const uint4*>(f->records); b.brick_of = f->brick_of; b.n_bricks = (long long)f->n_bricks;
    for (int c = 0; c < 3; ++c) b.R[c] = f->resolution[c];
    b.L = f->brick_log2; b.By = B[1]; b.Bz = B[2]; b.nch = rec_bytes(f->sh_degree) / 16;
}

static bool check_threshold(float t) { return t >= 0.f && std::isfinite(t); }

}  // namespace baked_bricks_grow
}  // namespace knerf

using namespace knerf;

extern "C" int knerf_baked_resample_bricks_sigma(void* stream, const knerf_baked_bricks* src, const int32_t dst_resolution[3],
                                                 float sigma_threshold, float* dst_sigma) {
    int B[3];
    if (!baked_bricks_grow::check_bricks(src, true, B) || !dst_resolution || !dst_sigma) return KNERF_ERR_INVALID;
    unsigned long long points_new = 0;
    if (!baked::check_lattice(dst_resolution, src->lo, src->hi, src->sh_degree, nullptr, points_new)) return KNERF_ERR_INVALID;   // (the same box)
    if (!baked_bricks_grow::check_threshold(sigma_threshold)) return KNERF_ERR_INVALID;
    baked_bricks_grow::SigmaArgs a{};
    baked_bricks_grow::set_bricks(a.src, src, B);
    a.dst = dst_sigma; a.n_new = (long long)points_new; a.threshold = sigma_threshold;
    for (int c = 0; c < 3; ++c) a.Rn[c] = dst_resolution[c];
    const unsigned long long blocks = (points_new + baked::kBlock - 1) / baked::kBlock;
    if (blocks >= (1ull << 31)) return KNERF_ERR_INVALID;
    hipLaunchKernelGGL(baked_bricks_grow::baked_bricks_sigma_kernel, dim3((unsigned)blocks), dim3(baked::kBlock), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_resample_bricks(void* stream, const knerf_baked_bricks* src, const knerf_baked_bricks* dst, const int32_t* dst_keys,
                                           float sigma_threshold, void* dst_records) {
    int B[3], Bd[3];
    if (!baked_bricks_grow::check_bricks(src, true, B) || !baked_bricks_grow::check_bricks(dst, false, Bd)) return KNERF_ERR_INVALID;
    if (!dst_keys || !dst_records) return KNERF_ERR_INVALID;
    if (dst->sh_degree != src->sh_degree) return KNERF_ERR_INVALID;
    for (int c = 0; c < 3; ++c)
        if (dst->lo[c] != src->lo[c] || dst->hi[c] != src->hi[c]) return KNERF_ERR_INVALID;      // the same box
    if (!baked_bricks_grow::check_threshold(sigma_threshold)) return KNERF_ERR_INVALID;
    const int deg = src->sh_degree;
    const unsigned long long rb = (unsigned)baked::rec_bytes(deg);
    const unsigned long long n_src = src->n_bricks << (3 * src->brick_log2), n_dst = dst->n_bricks << (3 * dst->brick_log2);
    const uintptr_t s0 = (uintptr_t)src->records, d0 = (uintptr_t)dst_records;
    if (s0 < d0 + n_dst * rb && d0 < s0 + n_src * rb) return KNERF_ERR_INVALID;                  // the record sets overlap
    baked_bricks_grow::ResampleArgs a{};
    baked_bricks_grow::set_bricks(a.src, src, B);
    a.dst = static_cast<uint4*>(dst_records); a.keys = dst_keys;
    a.n_records = (long long)n_dst; a.grid = (long long)Bd[0] * Bd[1] * Bd[2];
    for (int c = 0; c < 3; ++c) a.Rn[c] = dst->resolution[c];
    a.L = dst->brick_log2; a.By = Bd[1]; a.Bz = Bd[2]; a.K = baked::n_coeff(deg);
    a.threshold = sigma_threshold;
    const unsigned long long blocks = (n_dst * (unsigned)a.src.nch + baked::kBlock - 1) / baked::kBlock;
    if (blocks >= (1ull << 31)) return KNERF_ERR_INVALID;
    hipLaunchKernelGGL(baked_bricks_grow::baked_bricks_resample_kernel, dim3((unsigned)blocks), dim3(baked::kBlock), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

extern "C" int knerf_baked_bricks_train_tv(void* stream, const knerf_baked_bricks_train* train, const int32_t* keys, const uint8_t* flags,
                                           const float* master, float weight_sigma, float weight_sh, float epsilon, float* tv_out) {
    int B[3];
    // the struct errors of knerf_baked_bricks_train_apply
    if (!train || !train->field.bits || !train->grad || !baked_bricks_grow::check_bricks(&train->field, true, B)) return KNERF_ERR_INVALID;
    if (!keys || !flags || !master) return KNERF_ERR_INVALID;
    if (!baked_grow::check_tv(weight_sigma, weight_sh, epsilon)) return KNERF_ERR_INVALID;
    if (weight_sigma == 0.f && weight_sh == 0.f && !tv_out) return KNERF_OK;      // nothing to add, nothing to report
    const knerf_baked_bricks* f = &train->field;
    baked_bricks_grow::TvArgs a{};
    a.brick_of = f->brick_of; a.keys = keys; a.flags = flags; a.master = master; a.grad = train->grad; a.tv_out = tv_out;
    a.n_bricks = (long long)f->n_bricks; a.n_records = (long long)(f->n_bricks << (3 * f->brick_log2));
    a.grid = (long long)B[0] * B[1] * B[2];
    for (int c = 0; c < 3; ++c) a.R[c] = f->resolution[c];
    a.L = f->brick_log2; a.By = B[1]; a.Bz = B[2];
    a.w_sigma = weight_sigma; a.w_sh = weight_sh; a.eps = epsilon;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipErrorInvalidValue;
    switch (f->sh_degree) {
        case 0: e = baked_bricks_grow::launch_tv<4>(a, s); break;
        case 1: e = baked_bricks_grow::launch_tv<13>(a, s); break;
        case 2: e = baked_bricks_grow::launch_tv<28>(a, s); break;
        case 3: e = baked_bricks_grow::launch_tv<49>(a, s); break;
    }
    return e == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}
