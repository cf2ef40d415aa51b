// query.h -- launch interface of the fused point / grid query kernel (csrc/query.hip); internal, used by knerf_api.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace knerf {

struct QueryArgs {
    const char* stream;     // this net's packed forward A-fragments (the render path's stream, knerf_ctx::Net)
    const float* bias;      // kFwdBiasTiles*32 fp32
    const float* xyz;       // points mode: [n,3]; grid mode: null
    const float* dir;       // null (zero direction), [3] shared (dir_stride 0) or [n,3] (dir_stride 3)
    int dir_stride;
    int grid;               // 1: point g is (i,j,k) of a [gr0, gr1, gr2] grid (C order), at lo + idx * step per axis
    int gr[3];
    float lo[3], step[3];
    float* raw;             // [n,4] (r,g,b,sigma) or null
    float* sigma;           // [n] or null
    float* rgb;             // [n,3] or null
    long long n;
    long long offset;       // first point of this launch (grid and points mode alike)
    int shape;              // layout.h fused_shape_id
    // list mode (launch_query_list, the render pass behind an occupancy grid, csrc/occupancy.hip): sample gi = list[g] of a pass of
    // n = R*S samples, g < *count (device); ray gi / S, p = o + d * t[gi] as mlp_fwd.hip, direction d of the ray; writes raw[gi]
    const int* list;
    const int* count;
    const float* o;         // [R,3]
    const float* d;         // [R,3]
    const float* t;         // [R,S]
    int S;
};
hipError_t launch_query(const QueryArgs& a, hipStream_t stream);
template <class S> hipError_t launch_query_t(const QueryArgs& a, hipStream_t stream);
// list mode: a grid sized for all n samples; workgroups whose first list entry lies at or beyond *count exit at once (no host sync)
hipError_t launch_query_list(const QueryArgs& a, hipStream_t stream);
template <class S> hipError_t launch_query_list_t(const QueryArgs& a, hipStream_t stream);

// the general-shape route's prologue / epilogue (query.hip): points [n,3] and directions [n,3] of points offset .. offset+n-1,
// and raw [n,4] -> the caller's outputs at offset
hipError_t launch_query_gather(const QueryArgs& a, long long n, float* xyz, float* dir, hipStream_t stream);
hipError_t launch_query_scatter(const QueryArgs& a, long long n, const float* raw, hipStream_t stream);

}  // namespace knerf
