// raygen.hip -- pinhole ray generation on device (gfx950).
//
// Restates RaysGenerator.__call__ (reference keras_nerf/data/rays.py:69-130): pixel-corner grid, camera vector
// ((x-W/2)/f, -(y-H/2)/f, -1), d = sum(cam[...,None,:] * R, -1) normalised, o = c2w[:3,3],
// t = clip(linspace(near,far,N) + noise*interval - interval/2, near, far), noise ~ U[0,1) (injected or Philox).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rays.h"

namespace knerf {

// one thread per (ray, sample); the ray part is recomputed per sample (cheap) to keep the stores coalesced
__global__ void raygen_kernel(RayGenArgs a) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)a.B * a.H * a.W * a.N;
    if (idx >= total) return;
    const int n = (int)(idx % a.N);
    const long long ray = idx / a.N;
    const int xpix = (int)(ray % a.W);
    const int ypix = (int)((ray / a.W) % a.H);
    const int b = (int)(ray / ((long long)a.W * a.H));
    const float* M = a.c2w + (size_t)b * 16;
    float u;
    if (a.noise) u = a.noise[idx];
    else {
        unsigned c[4] = {(unsigned)(n >> 2), (unsigned)ray, (unsigned)a.stream_id, 1u};
        philox4x32_10(c, a.seed);
        u = philox_uniform(c, n);
    }
    a.t[idx] = stratified_sample(n, a.N, a.near_, a.far_, u);
    if (n == 0) pixel_ray(M, xpix, ypix, a.W, a.H, a.focal, a.o + ray * 3, a.d + ray * 3);
}

hipError_t launch_raygen(const RayGenArgs& a, hipStream_t stream) {
    const long long total = (long long)a.B * a.H * a.W * a.N;
    hipLaunchKernelGGL(raygen_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace knerf
