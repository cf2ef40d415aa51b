// ctx.h -- the context object behind the C ABI (include/knerf.h).  Internal: shared by knerf_api.hip and by the
// diagnostics library (debug_api.hip -> libknerf_probe.so), which reads workspace pointers out of it for kernel-level tests.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/knerf.h"
#include "generic.h"
#include "layout.h"
#include "occupancy.h"

namespace knerf {

// The one owner of a device allocation: a pointer and its element count, freed by the destructor.  Converts to T* where a kernel
// argument is filled; size() / bytes() are what was allocated (no rounding up, no geometric growth).
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }      // (a struct of buffers returned by value: host_tables_of)
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; n_ = 0;
    }
    // Room for n elements.  Fits: nothing happens (no allocation, free or synchronise).  Otherwise the old buffer goes -- after a
    // synchronise of `s`: nothing enqueued earlier may still use it -- and exactly n elements are allocated; the buffer reads
    // {null, 0} while hipMalloc runs and after it failed, so a failed allocation leaves a consistent owner.  zero: the fill is
    // enqueued on `s`, the stream the consuming kernels run on.
    hipError_t grow(size_t n, hipStream_t s, bool zero = false) {
        if (n <= n_) return hipSuccess;
        if (p_) {
            if (hipError_t e = hipStreamSynchronize(s)) return e;
            reset();
        }
        T* p = nullptr;
        if (hipError_t e = hipMalloc(&p, n * sizeof(T))) return e;
        p_ = p; n_ = n;
        return zero ? hipMemsetAsync(p_, 0, n * sizeof(T), s) : hipSuccess;
    }
};
// a group of buffers that is re-sized together gives its memory back before the first of them is allocated again
template <class... B>
inline void release(B&... b) { (b.reset(), ...); }

struct Net {
    DevBuf<float> w, m, v;                              // w: kExtParamCount floats on the fused path (parameters + composed head)
    float *g = nullptr, *aux = nullptr;                 // point into knerf_ctx::grads / knerf_ctx::aux
    DevBuf<char> fwd_stream, bwd_stream;
    DevBuf<float> bias;
};

struct Tables {
    PackTables host;
    std::vector<int32_t> wgrad;        // concatenated per-job destination tables
    std::vector<int32_t> wgrad_off;    // kWgradJobs+1 offsets
    DevBuf<int> d_fwd, d_bias, d_bwd, d_wgrad, d_plan;
    int n_plan = 0;
};

// the general-shape path's buffers (generic.h): the owners behind a gen::Workspace / gen::NetDev, which stay plain views
struct GenWsBufs { DevBuf<unsigned short> act, dz; DevBuf<unsigned char> mask; DevBuf<float> zc; };
struct GenNetBufs { DevBuf<unsigned short> packed; DevBuf<float> head, gaux; };

// the packing / destination tables of layout.h for one trunk shape, built once per process and shape (host only)
template <class S>
inline void build_wgrad_tables(Tables& t) {
    auto tt = tensor_table<S>();
    t.wgrad.clear(); t.wgrad_off.clear();
    for (int jb = 0; jb < S::kWgradJobs; ++jb) {
        t.wgrad_off.push_back((int32_t)t.wgrad.size());
        const WgradJob J = wgrad_job<S>(jb);
        const int rows = J.n_it * 32 + 1, cols = J.n_ot * 32;     // last row = bias
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) t.wgrad.push_back(wgrad_dst<S>(tt, jb, r == rows - 1 ? -2 : r, c));
    }
    t.wgrad_off.push_back((int32_t)t.wgrad.size());
}
template <class S>
inline const Tables& host_tables_of() {
    static const Tables t = [] { Tables x; build_fwd<S>(x.host); build_bwd<S>(x.host); build_wgrad_tables<S>(x); return x; }();
    return t;
}
inline const Tables& host_tables(int shape_id = 0) {      // layout.h fused_shape_id
    switch (shape_id) {
#define KNERF_X(I, ...) case I: return host_tables_of<KNERF_SHAPE_T(__VA_ARGS__)>();
        KNERF_FUSED_SHAPES(KNERF_X)
#undef KNERF_X
        default: return host_tables_of<DefaultShape>();
    }
}

}  // namespace knerf

struct knerf_ctx {
    knerf_config cfg;
    std::string err;
    knerf::Net net[2];
    knerf::DevBuf<float> grads;        // [coarse | fine] flat gradient accumulators: the DP all-reduce operand
    knerf::DevBuf<float> aux;          // [coarse | fine] head accumulators (layout.h kAuxCount each), expanded into grads per batch
    knerf::Tables tab;
    int step = 0;
    knerf::DevBuf<int> d_flag;         // device: set by the finite check of the current step
    knerf::DevBuf<int> d_step;         // device: optimizer steps applied so far (Adam's t - 1 of the next step)
    knerf::DevBuf<float> d_lr_t;       // device: bias-corrected learning rate of the next step, derived from d_step on the device
    int* h_status = nullptr;           // pinned host: [0] number of skipped (non-finite) steps so far, written by the device
    int skipped_seen = 0;
    // optimizer options (knerf_set_optimizer; optim_ext.h).  opt_ext: some extension is active and knerf_apply_adam takes the
    // extended kernels; false (the default, and a constant schedule without clipping or decay): the plain kernels with cfg.lr.
    // Device side, allocated by the first call that needs it: d_opt_f = [0] fp32(weight_decay * lr(step)) of the next step, [1..] the
    // clip factors [2][kOptMaxTensors]; d_opt_partial = [2][opt_items] sums of squares; d_opt_tab = tensor offsets [n + 1], first item
    // of each tensor [n + 1], item begin [items], item end [items]
    knerf_optimizer opt = {};
    bool opt_ext = false;
    knerf::DevBuf<float> d_opt_f;
    knerf::DevBuf<double> d_opt_partial;
    knerf::DevBuf<int> d_opt_tab;
    int opt_tensors = 0, opt_items = 0;
    // the objective (knerf_set_objective; composite_ext.h).  obj_ext: the loss is not the squared error or a regulariser is on, and the
    // training passes' compositing goes to composite_ext.hip; false (the default, and mse with both weights 0): the plain kernel.
    // d_terms: device [2][4], the terms of the passes since the last knerf_train_batch began
    knerf_objective obj = {0, 0.f, 0.f, 0.f, 3};
    bool obj_ext = false;
    knerf::DevBuf<float> d_terms;
    int n_cu = 256;
    // general-shape MLP path (generic.h): used when the fused kernels do not cover the config's MLP shape (layout.h KNERF_FUSED_SHAPES)
    bool generic = false;
    bool mlp_only = false;              // created with KNERF_FLAG_ENCODED_WIDTHS: a stand-alone NeRFMLP (weights + knerf_mlp_call)
    int shape = 0;                      // fused path: layout.h fused_shape_id of the trunk
    knerf::ShapeInfo si = knerf::shape_info(0);
    int n_params = knerf::kParamCount;
    knerf::gen::Plan gplan;
    knerf::GenWsBufs gws_buf; knerf::gen::Workspace gws;          // (the views are filled when the owners are sized)
    knerf::GenNetBufs gnet_buf[2]; knerf::gen::NetDev gnet[2];
    // knerf_mlp_call (NeRFMLP.__call__ on encoded inputs): own plan / packed weights / workspace, also on a fused-path context
    knerf::gen::Plan call_plan; bool call_plan_ok = false;
    knerf::GenWsBufs call_ws_buf; knerf::gen::Workspace call_ws;
    knerf::GenNetBufs call_net_buf; knerf::gen::NetDev call_net;
    // knerf_query_points / knerf_query_grid on the general-shape route: per-chunk points, directions, encodings and raw (grow-only)
    knerf::DevBuf<float> query_tmp;
    // occupancy grids of the render passes (knerf_set_occupancy; occupancy.h): per net, bits owned by the context and the grid as the
    // kernels take it (grid.bits null: none attached; the allocation outlives a detach only until the next attach re-sizes it), and the
    // compaction workspace of the fused path (ballots, per-workgroup counts / offsets, the list of live samples and its length), sized
    // with the render workspace while a grid is attached (ws_occ_rays)
    struct Occ { knerf::DevBuf<unsigned> bits; knerf::OccGrid grid = {}; };
    Occ occ[2];
    knerf::DevBuf<char> occ_ws; int ws_occ_rays = 0;
    knerf::DevBuf<long long> occ_stats; // [net][2]: samples whose MLP output is live (occupied), samples considered
    // training behind the grids (option "occupancy_train"; train_list.h): the compacted raw / dL/draw of a training pass and their size in
    // rays, allocated only while the option is on and a grid is attached (the compaction workspace occ_ws then covers the training size too);
    // occ_train_stats as occ_stats, for the train passes
    bool occ_train = false;
    knerf::DevBuf<float> occ_raw_c, occ_draw_c; int ws_occ_train_rays = 0;
    knerf::DevBuf<long long> occ_train_stats;
    // early ray termination of the render passes (options "termination_threshold" / "termination_segment"; termination.h): eps (0 = off),
    // the segment length, the fused path's workspace (T, ballots, per-workgroup counts / offsets, the segment's list and its length),
    // sized only while eps > 0 (grow-only), and [net][2]: samples whose MLP output is kept, samples of those passes
    double term_eps = 0.0; int term_L = 32;
    knerf::DevBuf<char> term_ws;
    knerf::DevBuf<long long> term_stats;
    // run-time options (knerf_set_option)
    bool deterministic = false;         // per-workgroup partial sums + ordered second pass instead of fp32 atomics (wgrad, loss)
    bool skip_dead = true;              // dgrad / wgrad skip 32-sample tiles whose dL/d(rgb, sigma) is exactly zero (exact; +0.3 % when nothing is dead)
    int wgrad_group_max = 4;            // chunks per coarse weight-gradient launch of knerf_train_batch (1 = one launch per chunk)
    double wgrad_group_gb = 40.0;       // memory budget of those grouped workspaces
    int merge_rays = 4096;              // knerf_train_batch: consecutive chunks share launches of up to this many rays (0: off)
    int merge_render_rays = 65536;      // knerf_render_batch on the fused path (no saved tensors: 5 KB of workspace per ray); general-shape path: merge_rays
    int wgrad_cost[17] = {};            // workgroups per job ~ cost (build_wgrad_plan); filled from the job kinds at creation
    bool grad_diag = false;             // zero-gradient diagnostics of the last chunk (nerf.py:430-451; NeRF.compile(run_eagerly=True))
    knerf::DevBuf<float> diag_tmp;      // the earlier chunks' accumulated gradient while the last chunk runs alone
    knerf::DevBuf<unsigned long long> d_diag;
    long long* h_diag = nullptr;        // pinned: [0] coarse, [1] fine non-zero count of the last chunk's gradient, [2] steps published
    bool plan_dirty = false;
    int group_cache_rays = 0, group_cache_chunks = 0, group_cache = 0;   // wgrad_group_for memo (hipMemGetInfo is a driver call)
    // (ray_chunks, chunk count) whose MERGED launches did not fit in memory: later calls start from the caller's own chunks instead
    // of failing the same allocation again (train / render); how often a merge was given up (option "merge_fallbacks", read-only)
    int merge_fail_rays = 0, merge_fail_chunks = 0, rmerge_fail_rays = 0, rmerge_fail_chunks = 0, merge_fallbacks = 0;
    double ws_limit_gb = 0.0;           // option "workspace_limit_gb" (tests): a workspace request above it meets a REAL failing hipMalloc
    // workspaces (grow-only).  Inference buffers (raw, w_c, t_f, img_tmp) follow the largest chunk seen by any call; the training
    // buffers (draw, act, mask, dz, tile lists) follow the largest TRAINING chunk and group only, so that rendering with a larger
    // ray_chunks does not re-size them.
    int ws_rays = 0; bool ws_train = false;
    int ws_train_rays = 0;
    int ws_group = 1;                   // training workspaces hold this many chunks (knerf_train_batch: one wgrad launch per group)
    knerf::DevBuf<float> raw, draw, w_c, t_f, img_tmp, loss_tmp;
    knerf::DevBuf<char> act, mask, dz;
    // dead-tile skipping: per-tile flags of the training workspaces (composite.hip), the compacted list and its length, running
    // totals (live, all) of the tiles seen by the dgrad launches
    knerf::DevBuf<int> tile_flags, tile_list, tile_list_g, tile_count;   // tile_list_g: the list of a group of coarse passes
    // tile_count: a ring of counters, one per list; the whole ring is zeroed by ONE memset when a call takes its first counter (and
    // again should a call need more than the ring holds: its earlier consumers are already enqueued, the stream orders the memset)
    // Sized per call (ensure_tile_counters: a train_batch of C chunks in groups of G needs 2 C + ceil(C / G)), grow-only, so that a
    // call never wraps while a group's counter is still being appended to.
    static constexpr int kTileCounters = 4096;     // the ring's first size: tile_count.size() counters
    int tile_counter_next = 0;
    knerf::DevBuf<long long> tile_stats;    // [net][4]: live, total (dgrad launches of that net's passes), two guard counters
    // deterministic mode: per-workgroup weight-gradient slabs, per-workgroup loss terms, plan offsets of the jobs
    knerf::DevBuf<float> partial, loss_partial;
    knerf::DevBuf<int> d_job_wg0;
    // optional per-kernel timing with HIP events on the caller's stream (knerf_profile_*)
    bool prof_on = false;
    struct ProfRec { int id; hipEvent_t e0, e1; };
    std::vector<ProfRec> prof;
};
