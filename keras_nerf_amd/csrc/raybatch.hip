// raybatch.hip -- one training batch of rays drawn at random over all pixels of all views, on device (gfx950).
//
// Slot i of a batch holds pixel perm(seed, epoch)(first + i) of the dataset (rays.h PixelPerm: a keyed bijection of
// [0, V*H*W), so an epoch visits every pixel once), its ray exactly as raygen_kernel writes it (rays.h pixel_ray), freshly
// jittered sample positions and the pixel's colour.  One launch per train step; the host only passes the position.
#include <hip/hip_runtime.h>
#include "rays.h"

namespace knerf {

// one thread per (slot, sample): the t stores -- the only real traffic -- are coalesced; the permutation, the ray and the colour
// are worked out once per slot, by the thread of its first sample
__global__ void raybatch_kernel(RayBatchArgs a) {
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
    a.t[idx] = stratified_sample(n, a.N, a.near_, a.far_, u);
    if (n != 0) return;
    const unsigned long long pix = perm_apply(a.perm, a.first + (unsigned long long)slot);
    const unsigned long long hw = (unsigned long long)a.H * a.W;
    const unsigned long long v = pix / hw;
    const unsigned in_view = (unsigned)(pix - v * hw);          // H * W < 2^31 (checked by the caller)
    const int ypix = (int)(in_view / (unsigned)a.W), xpix = (int)(in_view % (unsigned)a.W);
    pixel_ray(a.c2w + v * 16, xpix, ypix, a.W, a.H, a.focal, a.o + (size_t)slot * 3, a.d + (size_t)slot * 3);
    const float* px = a.images + pix * (unsigned)a.C;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.target[(size_t)slot * 3 + c] = px[c];
    if (a.index) a.index[slot] = (long long)pix;
}

hipError_t launch_raybatch(const RayBatchArgs& a, hipStream_t stream) {
    const long long total = (long long)a.n_rays * a.N;
    hipLaunchKernelGGL(raybatch_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace knerf
