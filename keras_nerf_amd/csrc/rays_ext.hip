// rays_ext.hip -- ray generation under a ray model (rays_ext.h): NDC rays for forward-facing scenes, samples linear in disparity.
//
// The counterparts of raygen_kernel (all pixels of some views) and raybatch_kernel (pixels drawn at random over all views) with the
// same arguments plus a RayModel; pinhole rays with linear spacing come out bit-identical to the plain kernels.  The pipeline behind
// them is unchanged: it reads per-ray t arrays and unit directions only.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rays_ext.h"

namespace knerf {

// one thread per (ray, sample), the t stores coalesced.  Every sample of an NDC ray needs the ray's length L: the ray is recomputed
// per thread (as raygen_kernel does; a few dozen flops against one store), the thread of sample 0 writes it.
__global__ void raygen_ext_kernel(RayGenArgs a, RayModel m) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)a.B * a.H * a.W * a.N;
    if (idx >= total) return;
    const int n = (int)(idx % a.N);
    const long long ray = idx / a.N;
    const int xpix = (int)(ray % a.W);
    const int ypix = (int)((ray / a.W) % a.H);
    const int b = (int)(ray / ((long long)a.W * a.H));
    float u;
    if (a.noise) u = a.noise[idx];
    else {
        unsigned c[4] = {(unsigned)(n >> 2), (unsigned)ray, (unsigned)a.stream_id, 1u};
        philox4x32_10(c, a.seed);
        u = philox_uniform(c, n);
    }
    float o[3], d[3], L = 1.f;
    if (m.ndc || n == 0) L = model_ray(m, a.c2w + (size_t)b * 16, xpix, ypix, a.W, a.H, a.focal, o, d);
    a.t[idx] = model_sample(m, n, a.N, a.near_, a.far_, u, L);
    if (n != 0) return;
#pragma unroll
    for (int r = 0; r < 3; ++r) { a.o[ray * 3 + r] = o[r]; a.d[ray * 3 + r] = d[r]; }
}

// the same per slot of a ray batch; the permutation is evaluated by every thread that needs the ray (all of them under NDC, the
// thread of sample 0 otherwise), the colour and the index are written by the thread of sample 0
__global__ void raybatch_ext_kernel(RayBatchArgs a, RayModel m) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)a.n_rays * a.N) return;
    const int n = (int)(idx % a.N);
    const int slot = (int)(idx / a.N);
    float u;
    if (a.noise) u = a.noise[idx];
    else {
        unsigned c[4] = {(unsigned)(n >> 2), (unsigned)slot, (unsigned)a.noise_stream, 2u};
        philox4x32_10(c, a.seed);
        u = philox_uniform(c, n);
    }
    float o[3], d[3], L = 1.f;
    unsigned long long pix = 0;
    if (m.ndc || n == 0) {
        pix = perm_apply(a.perm, a.first + (unsigned long long)slot);
        const unsigned long long hw = (unsigned long long)a.H * a.W;
        const unsigned long long v = pix / hw;
        const unsigned in_view = (unsigned)(pix - v * hw);          // H * W < 2^31 (checked by the caller)
        const int ypix = (int)(in_view / (unsigned)a.W), xpix = (int)(in_view % (unsigned)a.W);
        L = model_ray(m, a.c2w + v * 16, xpix, ypix, a.W, a.H, a.focal, o, d);
    }
    a.t[idx] = model_sample(m, n, a.N, a.near_, a.far_, u, L);
    if (n != 0) return;
    const float* px = a.images + pix * (unsigned)a.C;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.o[(size_t)slot * 3 + c] = o[c]; a.d[(size_t)slot * 3 + c] = d[c];
        a.target[(size_t)slot * 3 + c] = px[c];
    }
    if (a.index) a.index[slot] = (long long)pix;
}

hipError_t launch_raygen_ext(const RayGenArgs& a, const RayModel& m, hipStream_t stream) {
    const long long total = (long long)a.B * a.H * a.W * a.N;
    hipLaunchKernelGGL(raygen_ext_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, m);
    return hipGetLastError();
}

hipError_t launch_raybatch_ext(const RayBatchArgs& a, const RayModel& m, hipStream_t stream) {
    const long long total = (long long)a.n_rays * a.N;
    hipLaunchKernelGGL(raybatch_ext_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, m);
    return hipGetLastError();
}

}  // namespace knerf
