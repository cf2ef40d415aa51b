// rays_cam.h -- camera models in front of the ray stage: full intrinsics (fx, fy, cx, cy), OpenCV radial /
// tangential lens distortion and the equidistant fisheye, per launch one model and either one camera or one camera per view.
// cam_ray is shared by the two kernels of rays_cam.hip (all pixels of some views; pixels drawn at random over all views) so that both
// write bit-identical rays for the same pixel; project_point is its forward direction.  The pose arithmetic is rays.h's camera_ray
// and the NDC map rays_ext.h's ndc_map: a pinhole camera with fx = fy = focal, cx = W/2, cy = H/2 and pixel_offset 0 writes the
// plain kernels' bits.
//
// An intrinsics row is 12 floats: fx, fy, cx, cy, c0..c5, 0, 0
//   OPENCV   c = k1, k2, p1, p2, k3, 0        FISHEYE (equidistant)   c = k1, k2, k3, k4, 0, 0
// fx, fy > 0 and a lens that does not fold inside the image are the caller's to check (keras_nerf_amd/data/cameras.py
// check_invertible): the device cannot refuse them without a synchronisation.
#pragma once
#include <hip/hip_runtime.h>
#include "rays_ext.h"

namespace knerf {

constexpr int kCamPinhole = 0, kCamOpenCV = 1, kCamFisheye = 2;
constexpr int kCamRow = 12;            // floats per intrinsics row
constexpr int kCamNewtonSteps = 8;     // fixed: no data-dependent exit, every lane does the same work and results are reproducible

struct CamArgs {
    const float* intr;      // [n_cameras, 12] (device)
    int per_view;           // 0: row 0 for every view, 1: row v for view v
    float pixel_offset;     // added to the integer pixel coordinates: 0 = pixel corners (the plain camera), 0.5 = pixel centres
};

// OpenCV's distortion of normalised coordinates and, with jac, its Jacobian (a b; c d) = d(fx, fy) / d(x, y)
__device__ __forceinline__ void opencv_distort(const float* c, float x, float y, float& fx, float& fy, float* jac) {
    const float k1 = c[0], k2 = c[1], p1 = c[2], p2 = c[3], k3 = c[4];
    const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), xy = __fmul_rn(x, y);
    const float r2 = __fadd_rn(xx, yy);
    // rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
    const float rad = __fadd_rn(1.f, __fmul_rn(r2, __fadd_rn(k1, __fmul_rn(r2, __fadd_rn(k2, __fmul_rn(r2, k3))))));
    fx = __fadd_rn(__fadd_rn(__fmul_rn(x, rad), __fmul_rn(__fmul_rn(2.f, p1), xy)), __fmul_rn(p2, __fadd_rn(r2, __fmul_rn(2.f, xx))));
    fy = __fadd_rn(__fadd_rn(__fmul_rn(y, rad), __fmul_rn(p1, __fadd_rn(r2, __fmul_rn(2.f, yy)))), __fmul_rn(__fmul_rn(2.f, p2), xy));
    if (!jac) return;
    // d rad / d r2 = k1 + r2 (2 k2 + 3 k3 r2)
    const float dr = __fadd_rn(k1, __fmul_rn(r2, __fadd_rn(__fmul_rn(2.f, k2), __fmul_rn(__fmul_rn(3.f, k3), r2))));
    const float dr2 = __fmul_rn(2.f, dr);
    const float off = __fadd_rn(__fmul_rn(dr2, xy), __fmul_rn(2.f, __fadd_rn(__fmul_rn(p1, x), __fmul_rn(p2, y))));
    jac[0] = __fadd_rn(__fadd_rn(rad, __fmul_rn(dr2, xx)), __fadd_rn(__fmul_rn(__fmul_rn(2.f, p1), y), __fmul_rn(__fmul_rn(6.f, p2), x)));
    jac[1] = off;
    jac[2] = off;
    jac[3] = __fadd_rn(__fadd_rn(rad, __fmul_rn(dr2, yy)), __fadd_rn(__fmul_rn(__fmul_rn(6.f, p1), y), __fmul_rn(__fmul_rn(2.f, p2), x)));
}

// solve distort(xu, yu) = (xn, yn): 2-D Newton with the analytic Jacobian from (xn, yn)
__device__ __forceinline__ void opencv_undistort(const float* c, float xn, float yn, float& xu, float& yu) {
    float x = xn, y = yn;
#pragma unroll
    for (int i = 0; i < kCamNewtonSteps; ++i) {
        float fx, fy, j[4];
        opencv_distort(c, x, y, fx, fy, j);
        const float ex = __fsub_rn(fx, xn), ey = __fsub_rn(fy, yn);
        const float det = __fsub_rn(__fmul_rn(j[0], j[3]), __fmul_rn(j[1], j[2]));
        x = __fsub_rn(x, __fdiv_rn(__fsub_rn(__fmul_rn(j[3], ex), __fmul_rn(j[1], ey)), det));
        y = __fsub_rn(y, __fdiv_rn(__fsub_rn(__fmul_rn(j[0], ey), __fmul_rn(j[2], ex)), det));
    }
    xu = x; yu = y;
}

// the equidistant fisheye's theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) and, with slope, d theta_d / d theta
__device__ __forceinline__ float fisheye_distort(const float* c, float th, float* slope) {
    const float k1 = c[0], k2 = c[1], k3 = c[2], k4 = c[3];
    const float t2 = __fmul_rn(th, th);
    const float poly = __fadd_rn(1.f, __fmul_rn(t2, __fadd_rn(k1, __fmul_rn(t2, __fadd_rn(k2, __fmul_rn(t2, __fadd_rn(k3, __fmul_rn(t2, k4))))))));
    if (slope)
        *slope = __fadd_rn(1.f, __fmul_rn(t2, __fadd_rn(__fmul_rn(3.f, k1), __fmul_rn(t2, __fadd_rn(__fmul_rn(5.f, k2),
                     __fmul_rn(t2, __fadd_rn(__fmul_rn(7.f, k3), __fmul_rn(t2, __fmul_rn(9.f, k4)))))))));
    return __fmul_rn(th, poly);
}

// solve fisheye_distort(theta) = theta_d: 1-D Newton from theta_d
__device__ __forceinline__ float fisheye_undistort(const float* c, float thd) {
    float th = thd;
#pragma unroll
    for (int i = 0; i < kCamNewtonSteps; ++i) {
        float slope;
        const float f = fisheye_distort(c, th, &slope);
        th = __fsub_rn(th, __fdiv_rn(__fsub_rn(f, thd), slope));
    }
    return th;
}

// The ray of pixel (xpix, ypix) under intrinsics row k and pose M: distorted normalised coordinates, image y pointing down,
//   xn = (x + pixel_offset - cx) / fx,  yn = (y + pixel_offset - cy) / fy
// undistorted by the model, the camera vector (xu, -yu, -1) -- for the fisheye (sin th xn/thd, -sin th yn/thd, -cos th), valid past
// 90 degrees -- through camera_ray.
template <int MODEL>
__device__ __forceinline__ void cam_ray(const float* k, float pixel_offset, const float* M, int xpix, int ypix, float* o, float* d) {
    const float xn = __fdiv_rn(__fsub_rn(__fadd_rn((float)xpix, pixel_offset), k[2]), k[0]);
    const float yn = __fdiv_rn(__fsub_rn(__fadd_rn((float)ypix, pixel_offset), k[3]), k[1]);
    float cam[3];
    if (MODEL == kCamFisheye) {
        const float thd = sqrtf(__fadd_rn(__fmul_rn(xn, xn), __fmul_rn(yn, yn)));
        const float th = fisheye_undistort(k + 4, thd);
        const float s = thd > 0.f ? __fdiv_rn(sinf(th), thd) : 0.f;
        cam[0] = __fmul_rn(s, xn); cam[1] = -__fmul_rn(s, yn); cam[2] = thd > 0.f ? -cosf(th) : -1.f;
    } else {
        float xu = xn, yu = yn;
        if (MODEL == kCamOpenCV) opencv_undistort(k + 4, xn, yn, xu, yu);
        cam[0] = xu; cam[1] = -yu; cam[2] = -1.f;
    }
    camera_ray(M, cam, o, d);
}

// cam_ray under a ray model: with m.ndc the NDC image of the camera's ray, scales from the row's fx, fy.  Returns the NDC length.
template <int MODEL>
__device__ __forceinline__ float cam_model_ray(const RayModel& m, const float* k, float pixel_offset, const float* M, int xpix, int ypix,
                                               int W, int H, float* o, float* d) {
    cam_ray<MODEL>(k, pixel_offset, M, xpix, ypix, o, d);
    if (!m.ndc) return 1.f;
    return ndc_map(o, d, ndc_scale(k[0], W), ndc_scale(k[1], H), m.ndc_near);
}

struct ProjectArgs {
    const float* points;    // [n,3]
    const int* view;        // [n] or null: view 0
    const float* c2w;       // [V,4,4]
    CamArgs cam;
    unsigned long long n;
    float* pixels;          // [n,2]
    float* depth;           // [n]
    unsigned char* valid;   // [n]
};

hipError_t launch_raygen_cam(const RayGenArgs& a, const RayModel& m, const CamArgs& c, int model, hipStream_t stream);
hipError_t launch_raybatch_cam(const RayBatchArgs& a, const RayModel& m, const CamArgs& c, int model, hipStream_t stream);
hipError_t launch_project_points(const ProjectArgs& a, int model, hipStream_t stream);

}  // namespace knerf
