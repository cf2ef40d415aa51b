// occupancy.h -- launch interface of the occupancy-grid kernels (csrc/occupancy.hip); internal, used by knerf_api.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace knerf {

// one net's grid: cells[0] x cells[1] x cells[2] bits over [lo, lo + cells / scale], bit (i*cy + j)*cz + k of little-endian uint32
// words; scale = fp32(cells / (hi - lo)) (rounded once from double on the host)
struct OccGrid {
    const unsigned* bits;
    int cells[3];
    float lo[3], scale[3];
    int outside_empty;      // a sample outside the box: 0 = occupied, 1 = empty
};

// the cell lookup (include/knerf.h; occupancy.hip and termination.hip): outside if u < 0, floor(u) >= c or u is NaN on any axis.  floor(u) >= c <=> u >= c for an
// integer c, so no out-of-range float -> int conversion happens.
__device__ __forceinline__ bool occ_lookup(const OccGrid& G, float px, float py, float pz) {
    const float p[3] = {px, py, pz};
    int idx[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float u = __fmul_rn(__fsub_rn(p[c], G.lo[c]), G.scale[c]);
        if (!(u >= 0.f) || u >= (float)G.cells[c]) return !G.outside_empty;
        idx[c] = (int)__builtin_floorf(u);
    }
    const unsigned b = ((unsigned)idx[0] * (unsigned)G.cells[1] + (unsigned)idx[1]) * (unsigned)G.cells[2] + (unsigned)idx[2];
    return (G.bits[b >> 5] >> (b & 31u)) & 1u;
}

constexpr int kOccBlock = 256, kOccPer = 8, kOccSpan = kOccBlock * kOccPer;     // samples per workgroup of the mark / emit kernels

inline long long occ_blocks(long long n) { return (n + kOccSpan - 1) / kOccSpan; }

struct OccArgs {
    OccGrid grid;
    const float* o;         // [R,3]
    const float* d;         // [R,3]
    const float* t;         // [R,S]
    long long n;            // R*S samples of the pass
    int S;
    float* raw;             // [n,4]: the dead samples get (0, 0, 0, 0)
    unsigned long long* masks;   // [ceil(n / 64)] one ballot per 64 samples (null: no list wanted)
    int* blk_cnt;           // [occ_blocks(n)] live samples per workgroup (null with masks)
    int* blk_off;           // [occ_blocks(n)] exclusive prefix of blk_cnt
    int* list;              // [n] ascending live sample indices
    int* count;             // [1] its length
    long long* stats;       // [0] += live, [1] += n
};

// mark: cell lookup of every sample, raw = 0 at the dead ones, ballots and per-workgroup counts, stats.  With masks set, also the
// ordered compaction (scan of the counts, then the list) into list / count.
hipError_t launch_occupancy_mark(const OccArgs& a, hipStream_t stream);
// the one-workgroup exclusive scan of the mark step alone: off[b] = sum of cnt[< b], *count = the total (csrc/termination.hip)
hipError_t launch_occupancy_scan(const int* cnt, int nblk, int* off, int* count, hipStream_t stream);
// lattice sigma [rx,ry,rz] -> bits of the (rx-1) x (ry-1) x (rz-1) cells: occupied if a corner has sigma > threshold, then dilated
hipError_t launch_occupancy_build(const float* sigma, int rx, int ry, int rz, float threshold, int dilation, unsigned* bits, hipStream_t stream);

}  // namespace knerf
