// rays_ext.h -- ray models beyond the plain pinhole ray with samples linear in depth: normalised-device-coordinate (NDC) rays for
// forward-facing scenes and samples linear in disparity.  model_ray and model_sample are shared by the two
// kernels of rays_ext.hip (all pixels of some views; pixels drawn at random over all views), so that both write bit-identical rays for
// the same pixel -- the invariant rays.h keeps for the plain kernels, whose arithmetic (pixel_ray, stratified_sample, the Philox
// counters) is used here unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include "rays.h"

namespace knerf {

struct RayModel { int ndc; int spacing; float ndc_near; };   // spacing: 0 linear, 1 disparity
constexpr int kSpacingLinear = 0, kSpacingDisparity = 1;

// The NDC image of a ray (o, d) of a camera that looks along -z, with the near plane at distance n in front of it and the scales
// ax = -2 fx / W, ay = -2 fy / H of the camera (fx = fy = focal for the plain camera):
//   origin moved onto the near plane        s = -(n + o_z) / d_z,  o <- o + s d
//   o' = (ax o_x/o_z, ay o_y/o_z, 1 + 2n/o_z)
//   d' = (ax (d_x/d_z - o_x/o_z), ay (d_y/d_z - o_y/o_z), -2n/o_z)
// Overwrites o with o' and d with the UNIT direction d' / L, returns L = |d'|: o'_z = -1 and (o' + L d'/L)_z = +1, so t in [0, L]
// runs from the near plane to infinity.  Shared with rays_cam.h, whose cameras hand in their own rays and scales.
__device__ __forceinline__ float ndc_map(float* o, float* d, float ax, float ay, float n) {
    const float s = __fdiv_rn(-__fadd_rn(n, o[2]), d[2]);
    const float ox = __fadd_rn(o[0], __fmul_rn(s, d[0])), oy = __fadd_rn(o[1], __fmul_rn(s, d[1])), oz = __fadd_rn(o[2], __fmul_rn(s, d[2]));
    const float xz = __fdiv_rn(ox, oz), yz = __fdiv_rn(oy, oz), nz = __fdiv_rn(__fmul_rn(2.f, n), oz);
    const float dx = __fmul_rn(ax, __fsub_rn(__fdiv_rn(d[0], d[2]), xz));
    const float dy = __fmul_rn(ay, __fsub_rn(__fdiv_rn(d[1], d[2]), yz));
    const float dz = -nz;
    const float L = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
    o[0] = __fmul_rn(ax, xz); o[1] = __fmul_rn(ay, yz); o[2] = __fadd_rn(1.f, nz);
    d[0] = __fdiv_rn(dx, L); d[1] = __fdiv_rn(dy, L); d[2] = __fdiv_rn(dz, L);
    return L;
}

// the NDC scale of an axis: -2 f / extent
__device__ __forceinline__ float ndc_scale(float focal, int extent) { return -__fdiv_rn(__fmul_rn(2.f, focal), (float)extent); }

// The ray of pixel (xpix, ypix): pixel_ray's origin and unit direction; with m.ndc mapped to NDC space (ndc_map) with the near plane
// at distance m.ndc_near.  Returns the NDC length L (1 for a pinhole ray).
__device__ __forceinline__ float model_ray(const RayModel& m, const float* M, int xpix, int ypix, int W, int H, float focal,
                                           float* o, float* d) {
    pixel_ray(M, xpix, ypix, W, H, focal, o, d);
    if (!m.ndc) return 1.f;
    return ndc_map(o, d, ndc_scale(focal, W), ndc_scale(focal, H), m.ndc_near);
}

// sample position n of N of a ray of NDC length L (model_ray), from the uniform u of the plain kernels:
//   pinhole, linear     t = stratified_sample(n, N, near, far, u)                       (the plain kernels' value, bit for bit)
//   pinhole, disparity  s = stratified_sample(n, N, 0, 1, u), t = 1 / ((1 - s) / near + s / far)      (monotone in s)
//   NDC                 s = stratified_sample(n, N, near, far, u) with [near, far] inside [0, 1], t = s L
__device__ __forceinline__ float model_sample(const RayModel& m, int n, int N, float near_, float far_, float u, float L) {
    if (m.ndc) return __fmul_rn(stratified_sample(n, N, near_, far_, u), L);
    if (m.spacing == kSpacingDisparity) {
        const float s = stratified_sample(n, N, 0.f, 1.f, u);
        return __fdiv_rn(1.f, __fadd_rn(__fdiv_rn(__fsub_rn(1.f, s), near_), __fdiv_rn(s, far_)));
    }
    return stratified_sample(n, N, near_, far_, u);
}

struct RayGenArgs;       // kernels.h
hipError_t launch_raygen_ext(const RayGenArgs& a, const RayModel& m, hipStream_t stream);
hipError_t launch_raybatch_ext(const RayBatchArgs& a, const RayModel& m, hipStream_t stream);

}  // namespace knerf
