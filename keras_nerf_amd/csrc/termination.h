// termination.h -- launch interface of the early-ray-termination kernels (csrc/termination.hip); internal, used by knerf_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "occupancy.h"

namespace knerf {

// samples per workgroup of the mark / emit kernels: whole rays' segments, at most kTermSpan samples (rays_per_block(L) rays of L)
constexpr int kTermBlock = 256, kTermSpan = 2048, kTermWords = kTermSpan / 64;

inline int term_rays_per_block(int L) { return L >= kTermSpan ? 1 : kTermSpan / L; }
inline long long term_blocks(long long R, int L) { const int r = term_rays_per_block(L); return (R + r - 1) / r; }

struct TermArgs {
    OccGrid grid;           // the net's grid (has_grid = 1) or nothing
    int has_grid;
    const float* o;         // [R,3]
    const float* d;         // [R,3]
    const float* t;         // [R,S]
    float* raw;             // [R*S,4]: the dead samples get (0, 0, 0, 0)
    int R, S, L;            // L: segment length (option "termination_segment")
    int k;                  // round: segment k = samples [k L, min((k+1) L, S)) of every ray
    float eps;              // option "termination_threshold" (rounded to fp32)
    float* T;               // [R] transmittance in front of segment k (the mark kernel folds segment k - 1 into it)
    unsigned long long* masks;   // [term_blocks * kTermWords] per-workgroup ballots of segment k's live samples
    int* blk_cnt;           // [term_blocks] live samples per workgroup
    int* blk_off;           // [term_blocks] exclusive prefix of blk_cnt
    int* list;              // [R*L] ascending global sample indices (ray*S + i) of segment k's live samples
    int* count;             // [1] its length
    long long* occ_stats;   // null, or the net's [live, total] of knerf_occupancy_stats (the grid's verdict on every sample)
    long long* stats;       // the net's [evaluated, total] of knerf_termination_stats
};

// one round of the fused path: mark (fold segment k - 1 into T, cut, grid, raw = 0 at the dead samples, ballots), scan, emit.  The
// caller then runs launch_query_list over R * L_k samples (the list's length stays on the device).
hipError_t launch_termination_round(const TermArgs& a, hipStream_t stream);
// the general-shape path, behind its dense forward (and the grid's zeroing): one thread per ray walks the segments with the same cut
// rule and zeroes the terminated samples; stats as the fused path (list / masks unused)
hipError_t launch_termination_walk(const TermArgs& a, hipStream_t stream);

}  // namespace knerf
