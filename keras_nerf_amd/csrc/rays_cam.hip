// rays_cam.hip -- ray generation under a camera model (rays_cam.h): full intrinsics, OpenCV lens distortion, equidistant fisheye; and
// the forward projection of points into such cameras.
//
// The counterparts of raygen_ext_kernel and raybatch_ext_kernel (rays_ext.hip) with the same arguments, pixel order and Philox
// counters, the focal length replaced by an intrinsics table; templates on the camera model, so the pinhole instantiation carries no
// Newton code.  A pinhole camera with fx = fy = focal, cx = W/2, cy = H/2, pixel_offset 0 writes the bits of the plain kernels (of
// the _ext kernels under a ray model).  The pipeline behind them is unchanged: it reads per-ray t arrays and unit directions only.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rays_cam.h"

namespace knerf {

// one thread per (ray, sample), the t stores coalesced; the ray is computed by the thread of sample 0 and, under NDC, by every thread
// (each sample needs the ray's length L), as in rays_ext.hip
template <int MODEL>
__global__ void raygen_cam_kernel(RayGenArgs a, RayModel m, CamArgs cam) {
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
    if (m.ndc || n == 0) {
        const float* k = cam.intr + (cam.per_view ? (size_t)b * kCamRow : 0);
        L = cam_model_ray<MODEL>(m, k, cam.pixel_offset, a.c2w + (size_t)b * 16, xpix, ypix, a.W, a.H, o, d);
    }
    a.t[idx] = model_sample(m, n, a.N, a.near_, a.far_, u, L);
    if (n != 0) return;
#pragma unroll
    for (int r = 0; r < 3; ++r) { a.o[ray * 3 + r] = o[r]; a.d[ray * 3 + r] = d[r]; }
}

// the same per slot of a ray batch; the colour and the index are written by the thread of sample 0
template <int MODEL>
__global__ void raybatch_cam_kernel(RayBatchArgs a, RayModel m, CamArgs cam) {
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
        const unsigned long long v = pix / hw;                      // < n_views: perm_apply returns a value below P = n_views * hw
        const unsigned in_view = (unsigned)(pix - v * hw);          // H * W < 2^31 (checked by the caller)
        const int ypix = (int)(in_view / (unsigned)a.W), xpix = (int)(in_view % (unsigned)a.W);
        const float* k = cam.intr + (cam.per_view ? (size_t)v * kCamRow : 0);
        L = cam_model_ray<MODEL>(m, k, cam.pixel_offset, a.c2w + v * 16, xpix, ypix, a.W, a.H, o, d);
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

// The forward map, one lane per point, no iteration: the point in the camera's frame, p = R^T (x - t); depth = -p_z;
//   PINHOLE / OPENCV  (xu, yu) = (p_x, -p_y) / depth, distorted (OPENCV); valid: depth > 0
//   FISHEYE           theta = atan2(|p_xy|, depth), theta_d from the polynomial, (xn, yn) = theta_d (p_x, -p_y) / |p_xy|; valid: the
//                     point is not the camera centre and theta < pi
// pixel = (xn fx + cx - pixel_offset, yn fy + cy - pixel_offset): the coordinates the ray kernels take.
template <int MODEL>
__global__ void project_points_kernel(ProjectArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int v = a.view ? a.view[i] : 0;
    const float* M = a.c2w + (size_t)v * 16;
    const float* k = a.cam.intr + (a.cam.per_view ? (size_t)v * kCamRow : 0);
    float q[3], p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = __fsub_rn(a.points[i * 3 + r], M[r * 4 + 3]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        p[c] = __fadd_rn(__fadd_rn(__fmul_rn(M[0 * 4 + c], q[0]), __fmul_rn(M[1 * 4 + c], q[1])), __fmul_rn(M[2 * 4 + c], q[2]));
    const float depth = -p[2];
    float xn, yn;
    bool ok;
    if (MODEL == kCamFisheye) {
        const float r = sqrtf(__fadd_rn(__fmul_rn(p[0], p[0]), __fmul_rn(p[1], p[1])));
        const float th = atan2f(r, depth);
        const float thd = fisheye_distort(k + 4, th, nullptr);
        const float s = r > 0.f ? __fdiv_rn(thd, r) : 0.f;
        xn = __fmul_rn(s, p[0]); yn = -__fmul_rn(s, p[1]);
        ok = (r > 0.f || depth > 0.f) && th < 3.14159265358979323846f;
    } else {
        const float xu = __fdiv_rn(p[0], depth), yu = -__fdiv_rn(p[1], depth);
        xn = xu; yn = yu;
        if (MODEL == kCamOpenCV) opencv_distort(k + 4, xu, yu, xn, yn, nullptr);
        ok = depth > 0.f;
    }
    a.pixels[i * 2 + 0] = __fsub_rn(__fadd_rn(__fmul_rn(xn, k[0]), k[2]), a.cam.pixel_offset);
    a.pixels[i * 2 + 1] = __fsub_rn(__fadd_rn(__fmul_rn(yn, k[1]), k[3]), a.cam.pixel_offset);
    a.depth[i] = depth;
    a.valid[i] = ok ? 1 : 0;
}

hipError_t launch_raygen_cam(const RayGenArgs& a, const RayModel& m, const CamArgs& c, int model, hipStream_t stream) {
    const long long total = (long long)a.B * a.H * a.W * a.N;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    switch (model) {
        case kCamPinhole: hipLaunchKernelGGL(raygen_cam_kernel<kCamPinhole>, grid, block, 0, stream, a, m, c); break;
        case kCamOpenCV: hipLaunchKernelGGL(raygen_cam_kernel<kCamOpenCV>, grid, block, 0, stream, a, m, c); break;
        case kCamFisheye: hipLaunchKernelGGL(raygen_cam_kernel<kCamFisheye>, grid, block, 0, stream, a, m, c); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_raybatch_cam(const RayBatchArgs& a, const RayModel& m, const CamArgs& c, int model, hipStream_t stream) {
    const long long total = (long long)a.n_rays * a.N;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    switch (model) {
        case kCamPinhole: hipLaunchKernelGGL(raybatch_cam_kernel<kCamPinhole>, grid, block, 0, stream, a, m, c); break;
        case kCamOpenCV: hipLaunchKernelGGL(raybatch_cam_kernel<kCamOpenCV>, grid, block, 0, stream, a, m, c); break;
        case kCamFisheye: hipLaunchKernelGGL(raybatch_cam_kernel<kCamFisheye>, grid, block, 0, stream, a, m, c); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_project_points(const ProjectArgs& a, int model, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
    switch (model) {
        case kCamPinhole: hipLaunchKernelGGL(project_points_kernel<kCamPinhole>, grid, block, 0, stream, a); break;
        case kCamOpenCV: hipLaunchKernelGGL(project_points_kernel<kCamOpenCV>, grid, block, 0, stream, a); break;
        case kCamFisheye: hipLaunchKernelGGL(project_points_kernel<kCamFisheye>, grid, block, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace knerf
