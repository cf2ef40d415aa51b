// rays.h -- the per-pixel ray arithmetic and the counter-based generator shared by raygen.hip (all pixels of some views) and
// raybatch.hip (pixels drawn at random over all views), so that both write bit-identical rays for the same pixel.
//
// Philox-4x32-10 streams keyed by a seed; the fourth counter word names the consumer and keeps the streams apart:
//   0  sampler.hip   fine-sample u          1  raygen.hip   jitter of whole views
//   2  raybatch.hip  jitter of a ray batch  3  raybatch.hip round keys of the pixel permutation
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace knerf {

__host__ __device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
    const unsigned long long p0 = (unsigned long long)c[0] * 0xD2511F53ull;
    const unsigned long long p1 = (unsigned long long)c[2] * 0xCD9E8D57ull;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (unsigned)p1; c[3] = (unsigned)p0; c[0] = n0; c[2] = n2;
}

__host__ __device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned long long key) {
    unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
}

// one of the four words of a Philox block -> [0, 1) with 24 bits
__device__ __forceinline__ float philox_uniform(const unsigned (&c)[4], int lane) {
    return (float)(c[lane & 3] >> 8) * 5.9604644775390625e-08f;
}

// t[n] = clip(linspace(near, far, N)[n] + u * interval - interval / 2, near, far): linspace as TF computes it
// (start + n * ((stop - start) / (N - 1)), last point exact)
__device__ __forceinline__ float stratified_sample(int n, int N, float near_, float far_, float u) {
    const float step = N > 1 ? (far_ - near_) / (float)(N - 1) : 0.f;
    const float base = (n == N - 1 && N > 1) ? far_ : near_ + (float)n * step;
    const float interval = (far_ - near_) / (float)N;
    const float tv = __fsub_rn(__fadd_rn(base, __fmul_rn(u, interval)), interval / 2.f);
    return fminf(fmaxf(tv, near_), far_);
}

// the ray of a camera-space vector under pose M (c2w, 4x4 row-major): the vector rotated and normalised, origin = the translation
// column.  Every camera of the project ends here (pixel_ray below, rays_cam.h), so that they share these roundings.
__device__ __forceinline__ void camera_ray(const float* M, const float (&cam)[3], float* o, float* d) {
    float dv[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        dv[r] = __fadd_rn(__fadd_rn(__fmul_rn(cam[0], M[r * 4 + 0]), __fmul_rn(cam[1], M[r * 4 + 1])), __fmul_rn(cam[2], M[r * 4 + 2]));
    const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dv[0], dv[0]), __fmul_rn(dv[1], dv[1])), __fmul_rn(dv[2], dv[2])));
#pragma unroll
    for (int r = 0; r < 3; ++r) { d[r] = __fdiv_rn(dv[r], nrm); o[r] = M[r * 4 + 3]; }
}

// the ray through the corner of pixel (xpix, ypix) of a W x H pinhole camera with pose M (c2w, 4x4 row-major): camera vector
// ((x - W/2) / f, -(y - H/2) / f, -1) rotated and normalised, origin = the translation column
__device__ __forceinline__ void pixel_ray(const float* M, int xpix, int ypix, int W, int H, float focal, float* o, float* d) {
    const float xc = __fdiv_rn((float)xpix - (float)W * 0.5f, focal);
    const float yc = __fdiv_rn((float)ypix - (float)H * 0.5f, focal);
    const float cam[3] = {xc, -yc, -1.f};
    camera_ray(M, cam, o, d);
}

// ---- the pixel permutation of a ray batch: a keyed bijection of [0, P), evaluated per position, no table.
// A Feistel network over b = bit_length(P - 1) bits, split into a high half of b / 2 and a low half of b - b / 2 bits that swap
// places every round (six rounds, so the halves end where they began), cycle-walked until the value falls below P.  The domain
// 2^b is below 2 P, so a walk is short; it ends because it follows a cycle of a permutation that starts inside [0, P).
constexpr int kPermRounds = 6;

struct PixelPerm {
    unsigned long long P;
    int lo_bits, hi_bits;
    unsigned key[kPermRounds];
};

__host__ __device__ __forceinline__ unsigned fmix32(unsigned h) {      // the murmur3 finaliser
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

__host__ __device__ __forceinline__ unsigned long long perm_apply(const PixelPerm& p, unsigned long long pos) {
    unsigned long long x = pos;
    do {
        unsigned L = (unsigned)(x >> p.lo_bits), R = (unsigned)(x & ((1ull << p.lo_bits) - 1ull));
        int wl = p.hi_bits;
#pragma unroll
        for (int i = 0; i < kPermRounds; ++i) {
            const unsigned nr = (L ^ fmix32(R ^ p.key[i])) & ((1u << wl) - 1u);
            L = R; R = nr;
            wl = p.hi_bits + p.lo_bits - wl;
        }
        x = ((unsigned long long)L << p.lo_bits) | R;
    } while (x >= p.P);
    return x;
}

// round keys: two Philox blocks with counter (j, epoch lo, epoch hi, 3) under the key `seed`
inline PixelPerm make_pixel_perm(unsigned long long P, unsigned long long seed, unsigned long long epoch) {
    PixelPerm p{};
    p.P = P;
    int b = 0;
    while (b < 63 && ((P - 1) >> b)) ++b;
    p.hi_bits = b / 2; p.lo_bits = b - b / 2;
    for (unsigned j = 0; j < 2; ++j) {
        unsigned c[4] = {j, (unsigned)epoch, (unsigned)(epoch >> 32), 3u};
        philox4x32_10(c, seed);
        for (int i = 0; i < 4 && (int)j * 4 + i < kPermRounds; ++i) p.key[j * 4 + i] = c[i];
    }
    return p;
}

struct RayBatchArgs {
    const float* images;    // [V,H,W,C]
    const float* c2w;       // [V,4,4] row-major
    const float* noise;     // [n_rays,N] in [0,1) or null -> Philox
    float* o; float* d; float* t; float* target;
    long long* index;       // [n_rays] or null
    PixelPerm perm;
    unsigned long long first, seed, noise_stream;
    int n_rays, H, W, C, N;
    float focal, near_, far_;
};
hipError_t launch_raybatch(const RayBatchArgs& a, hipStream_t stream);

}  // namespace knerf
