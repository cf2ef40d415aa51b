// train_list.h -- launch interface of the list-mode training forward (csrc/train_list.hip); internal, used by knerf_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace knerf {

// The training forward of a pass behind an occupancy grid (knerf_set_option "occupancy_train"): compacted entry i < *count (device)
// is sample g = list[i] of the pass's f.n_samples = R*S samples; ray g / S, p = o + d * t[g] as mlp_fwd.hip.  The saved act / mask
// blocks go to compacted tile i / 32 (f.act / f.mask, the layout of mlp_fwd.hip), raw to f.raw[g] (what compositing reads).  The grid
// is sized for all f.n_samples entries; workgroups past the count exit at once.
struct TrainListArgs {
    FwdArgs f;
    const int* list;        // [n] ascending live sample indices (csrc/occupancy.hip mark / scan / emit)
    const int* count;       // [1] its length
};
hipError_t launch_mlp_fwd_list(const TrainListArgs& a, hipStream_t stream);
template <class S> hipError_t launch_mlp_fwd_list_t(const TrainListArgs& a, hipStream_t stream);

// After compositing, for the compacted backward: raw_c[i] = raw[list[i]] and draw_c[i] = draw[list[i]] for i < L = *count (what mlp_bwd
// reads); draw_c = raw_c = 0 on the rest of the
// last compacted tile; flags[j] for every tile j < n_tiles: 1 if j < ceil(L / 32) and (skip_dead == 0 or some draw_c of tile j is
// non-zero).  n: samples of the pass; n_tiles * 32 >= n.
hipError_t launch_occupancy_train_gather(const int* list, const int* count, const float* raw, const float* draw, float* draw_c, float* raw_c, int* flags,
                                         long long n, long long n_tiles, int skip_dead, hipStream_t stream);

}  // namespace knerf
