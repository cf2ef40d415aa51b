// mesh.hip -- marching cubes on a device fp32 density grid (gfx950), context-free.  Extension: the reference has no mesh export.
//
// Grid sigma[Rx][Ry][Rz] (C order, z fastest); point (i,j,k) lies at lo + idx * step per axis, step = (hi - lo) / (R - 1) in fp32,
// the coordinate __fadd_rn(lo, __fmul_rn(idx, step)) (csrc/query.hip places grid queries the same way).  A point is INSIDE when
// sigma > tau.  Grid edge e = 3 p + a joins point p to its neighbour along axis a; a crossed edge (exactly one end inside) carries
// ONE vertex, shared by the up to four cubes around it.  Cube p has point p as its corner 0 (csrc/mesh_table.h numbering).
//
// Pipeline (all on the caller's stream, one host read of the two totals):
//   1. edge_flag_kernel      vid[e] = 1 if edge e is crossed
//   2. exclusive scan        vid[e] = vertex id of edge e, V = total
//   3. cube_count_kernel     fcnt[p] = triangles of cube p (table count of its case)
//   4. exclusive scan        fcnt[p] = first face of cube p, F = total
//   5. vertex_emit_kernel / face_emit_kernel
// Output order is fixed by the scans (vertices by edge id, faces by cube then table order): two calls give identical arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/knerf.h"
#include "mesh_table.h"

namespace knerf {
namespace mc {

constexpr int kScanThreads = 256, kScanItems = 4, kScanBlock = kScanThreads * kScanItems;   // elements per scan block
constexpr long long kMaxPoints = 1ll << 28;        // 3 N edge ids and <= 12 N face indices stay inside uint32 / int32

struct Grid {
    const float* s;
    int rx, ry, rz;
    float lo[3], step[3];
    float tau;
    long long n;               // rx * ry * rz
};

__device__ __forceinline__ void unflatten(const Grid& g, long long p, int (&ix)[3]) {
    const long long yz = (long long)g.ry * g.rz;
    ix[0] = (int)(p / yz);
    const long long r = p - (long long)ix[0] * yz;
    ix[1] = (int)(r / g.rz);
    ix[2] = (int)(r - (long long)ix[1] * g.rz);
}
__device__ __forceinline__ long long flat(const Grid& g, int i, int j, int k) { return ((long long)i * g.ry + j) * g.rz + k; }
__device__ __forceinline__ int extent(const Grid& g, int a) { return a == 0 ? g.rx : (a == 1 ? g.ry : g.rz); }
__device__ __forceinline__ long long stride(const Grid& g, int a) { return a == 0 ? (long long)g.ry * g.rz : (a == 1 ? (long long)g.rz : 1ll); }
__device__ __forceinline__ float coord(const Grid& g, int a, int idx) { return __fadd_rn(g.lo[a], __fmul_rn((float)idx, g.step[a])); }

// edge e crossed?  (the far end must exist; exactly one end inside)
__device__ __forceinline__ bool crossed(const Grid& g, long long e, long long& p, int& a, int (&ix)[3]) {
    p = e / 3; a = (int)(e - 3 * p);
    unflatten(g, p, ix);
    if (ix[a] + 1 >= extent(g, a)) return false;
    return (g.s[p] > g.tau) != (g.s[p + stride(g, a)] > g.tau);
}

__global__ void edge_flag_kernel(Grid g, unsigned* vid) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3 * g.n) return;
    long long p; int a, ix[3];
    vid[e] = crossed(g, e, p, a, ix) ? 1u : 0u;
}

__device__ __forceinline__ int cube_case(const Grid& g, long long p, const int (&ix)[3]) {
    if (ix[0] + 1 >= g.rx || ix[1] + 1 >= g.ry || ix[2] + 1 >= g.rz) return -1;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long q = p + ((k & 1) ? stride(g, 0) : 0) + ((k & 2) ? stride(g, 1) : 0) + ((k & 4) ? 1 : 0);
        c |= (g.s[q] > g.tau ? 1 : 0) << k;
    }
    return c;
}

__global__ void cube_count_kernel(Grid g, unsigned* fcnt) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.n) return;
    int ix[3];
    unflatten(g, p, ix);
    const int c = cube_case(g, p, ix);
    fcnt[p] = c < 0 ? 0u : (unsigned)kTriCount[c];
}

// -grad sigma at point (ix) along axis b: central difference, one-sided at the border
__device__ __forceinline__ float grad(const Grid& g, long long p, const int (&ix)[3], int b) {
    const int lo = ix[b] > 0 ? ix[b] - 1 : 0, hi = ix[b] + 1 < extent(g, b) ? ix[b] + 1 : ix[b];
    const float d = __fsub_rn(g.s[p + (long long)(hi - ix[b]) * stride(g, b)], g.s[p - (long long)(ix[b] - lo) * stride(g, b)]);
    return __fdiv_rn(d, __fmul_rn((float)(hi - lo), g.step[b]));
}

__global__ void vertex_emit_kernel(Grid g, const unsigned* vid, float* vert, float* nrm) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3 * g.n) return;
    long long p; int a, ix[3];
    if (!crossed(g, e, p, a, ix)) return;
    const long long q = p + stride(g, a);
    const float sa = g.s[p], sb = g.s[q];
    const float t = __fdiv_rn(__fsub_rn(g.tau, sa), __fsub_rn(sb, sa));      // sb != sa: exactly one end is inside
    const long long v = vid[e];
    if (vert) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float pa = coord(g, b, ix[b]);
            vert[3 * v + b] = b == a ? __fadd_rn(pa, __fmul_rn(t, __fsub_rn(coord(g, b, ix[b] + 1), pa))) : pa;
        }
    }
    if (nrm) {
        int jx[3] = {ix[0], ix[1], ix[2]};
        jx[a] += 1;
        float n[3];
        const float u = __fsub_rn(1.f, t);
#pragma unroll
        for (int b = 0; b < 3; ++b) n[b] = -__fadd_rn(__fmul_rn(u, grad(g, p, ix, b)), __fmul_rn(t, grad(g, q, jx, b)));
        const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(n[0], n[0]), __fmul_rn(n[1], n[1])), __fmul_rn(n[2], n[2])));
#pragma unroll
        for (int b = 0; b < 3; ++b) nrm[3 * v + b] = len > 0.f ? __fdiv_rn(n[b], len) : 0.f;
    }
}

__global__ void face_emit_kernel(Grid g, const unsigned* vid, const unsigned* fofs, int* faces) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.n) return;
    int ix[3];
    unflatten(g, p, ix);
    const int c = cube_case(g, p, ix);
    if (c < 0) return;
    const int nt = kTriCount[c];
    const long long f0 = fofs[p];
    for (int t = 0; t < nt; ++t) {
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const int ce = kTris[c][3 * t + v];
            const int c0 = kEdge[ce][0], a = kEdge[ce][2];
            const long long pc = p + ((c0 & 1) ? stride(g, 0) : 0) + ((c0 & 2) ? stride(g, 1) : 0) + ((c0 & 4) ? 1 : 0);
            faces[3 * (f0 + t) + v] = (int)vid[3 * pc + a];
        }
    }
}

// ---- exclusive scan of uint32 (in place): per block of kScanBlock elements, then the block sums, recursively
__global__ __launch_bounds__(kScanThreads) void scan_block_kernel(unsigned* data, long long n, unsigned* sums, unsigned* total) {
    __shared__ unsigned wsum[kScanThreads / 64];
    const long long base = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kScanItems;
    unsigned v[kScanItems], s = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) { v[i] = base + i < n ? data[base + i] : 0u; s += v[i]; }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = s;                                     // inclusive scan of the thread sums inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kScanThreads / 64; ++k) { if (k < w) before += wsum[k]; all += wsum[k]; }
    unsigned run = before + inc - s;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        if (base + i < n) data[base + i] = run;
        run += v[i];
    }
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = all;
        if (gridDim.x == 1 && total) *total = all;
    }
}

__global__ void scan_add_kernel(unsigned* data, long long n, const unsigned* sums) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) data[i] += sums[i / kScanBlock];
}

long long blocks_of(long long n) { return (n + kScanBlock - 1) / kScanBlock; }

// scratch (uint32) a scan of n elements needs: the block sums of every level
long long scan_scratch(long long n) {
    long long s = 0;
    do { n = blocks_of(n); s += n; } while (n > 1);
    return s;
}

hipError_t scan(unsigned* data, long long n, unsigned* scratch, unsigned* total, hipStream_t st) {
    const long long nb = blocks_of(n);
    hipLaunchKernelGGL(scan_block_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, st, data, n, scratch, nb == 1 ? total : nullptr);
    if (hipError_t e = hipGetLastError()) return e;
    if (nb > 1) {
        if (hipError_t e = scan(scratch, nb, scratch + nb, total, st)) return e;
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, data, n, scratch);
        return hipGetLastError();
    }
    return hipSuccess;
}

// workspace: vid [3N] | fcnt [N] | totals [2] (+2 pad) | scan scratch of 3N elements (shared by both scans)
size_t ws_bytes(long long n) { return (size_t)(3 * n + n + 4 + scan_scratch(3 * n)) * sizeof(unsigned); }

}  // namespace mc
}  // namespace knerf

using namespace knerf;

extern "C" int knerf_marching_cubes(void* stream, const float* grid, int rx, int ry, int rz, const float* lo, const float* hi, float threshold,
                                    void* workspace, size_t* workspace_bytes, int64_t* counts, float* vertices, int32_t* faces, float* normals) {
    if (rx < 2 || ry < 2 || rz < 2 || !lo || !hi || !workspace_bytes) return KNERF_ERR_INVALID;
    const long long n = (long long)rx * ry * rz;
    if (n > mc::kMaxPoints) return KNERF_ERR_INVALID;
    const size_t need = mc::ws_bytes(n);
    if (!workspace) { *workspace_bytes = need; return KNERF_OK; }
    if (!grid || *workspace_bytes < need || !counts) return KNERF_ERR_INVALID;
    mc::Grid g{};
    g.s = grid; g.rx = rx; g.ry = ry; g.rz = rz; g.tau = threshold; g.n = n;
    const int R[3] = {rx, ry, rz};
    for (int a = 0; a < 3; ++a) {
        if (!(hi[a] > lo[a])) return KNERF_ERR_INVALID;
        g.lo[a] = lo[a];
        g.step[a] = (hi[a] - lo[a]) / (float)(R[a] - 1);         // fp32 subtraction and division (host SSE: correctly rounded)
    }
    unsigned* vid = static_cast<unsigned*>(workspace);
    unsigned* fcnt = vid + 3 * n;
    unsigned* totals = fcnt + n;
    unsigned* scratch = totals + 4;
    hipStream_t s = (hipStream_t)stream;
    const unsigned ge = (unsigned)((3 * n + 255) / 256), gp = (unsigned)((n + 255) / 256);
    if (!vertices && !faces && !normals) {         // count phase: classify, scan, read the two totals (the one host synchronisation)
        hipLaunchKernelGGL(mc::edge_flag_kernel, dim3(ge), dim3(256), 0, s, g, vid);
        if (hipGetLastError() != hipSuccess || mc::scan(vid, 3 * n, scratch, totals, s) != hipSuccess) return KNERF_ERR_HIP;
        hipLaunchKernelGGL(mc::cube_count_kernel, dim3(gp), dim3(256), 0, s, g, fcnt);
        if (hipGetLastError() != hipSuccess || mc::scan(fcnt, n, scratch, totals + 1, s) != hipSuccess) return KNERF_ERR_HIP;
        unsigned h[2];
        if (hipMemcpyAsync(h, totals, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return KNERF_ERR_HIP;
        counts[0] = h[0]; counts[1] = h[1];
        return KNERF_OK;
    }
    // emit phase: the workspace of the count phase on the same grid and threshold; arrays sized by its counts
    if (counts[0] > 0 && (vertices || normals)) {
        hipLaunchKernelGGL(mc::vertex_emit_kernel, dim3(ge), dim3(256), 0, s, g, vid, vertices, normals);
        if (hipGetLastError() != hipSuccess) return KNERF_ERR_HIP;
    }
    if (counts[1] > 0 && faces) {
        hipLaunchKernelGGL(mc::face_emit_kernel, dim3(gp), dim3(256), 0, s, g, vid, fcnt, faces);
        if (hipGetLastError() != hipSuccess) return KNERF_ERR_HIP;
    }
    return KNERF_OK;
}
