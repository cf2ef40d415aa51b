// knerf_api.hip -- extern "C" entry points of libknerf_hip.so (see include/knerf.h for the contract and the reference
// lines each one replaces).  Host-side only: owns device memory, sequences the kernels on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/knerf.h"
#include "chain.h"
#include "composite_ext.h"
#include "ctx.h"
#include "kernels.h"
#include "generic.h"
#include "layout.h"
#include "occupancy.h"
#include "optim_ext.h"
#include "query.h"
#include "rays.h"
#include "rays_ext.h"
#include "rays_cam.h"
#include "termination.h"
#include "train_list.h"

using namespace knerf;

#ifdef KNERF_N_SHAPE_SLICES
static_assert(KNERF_N_SHAPE_SLICES == kNumFusedShapes, "keras_nerf_amd/build.py N_SHAPE_SLICES must equal the number of entries of layout.h KNERF_FUSED_SHAPES");
#endif

namespace {

std::string g_create_error;

// Workgroups per wgrad job in proportion to the job's measured cost per sample tile (cycles per loop iteration from the
// s_memtime stamps of a -DKNERF_WGRAD_STAMPS build, tools/kbench.py): the streaming jobs are HBM-bound, the small ones
// (layer_0, head) latency-bound, so bytes alone mis-balance them.  About one workgroup per CU in total.
// knerf_set_option(ctx, "wgrad_cost<j>", c) overrides an entry (tuning sweeps in one gpurun call: tools/tune_costs.py).
// job_wg0[j] = index of job j's first workgroup (kWgradJobs + 1 entries): the deterministic mode's second pass walks them in order.
std::vector<int32_t> build_wgrad_plan(int n_wg, const int* cost, int n_jobs, std::vector<int32_t>& job_wg0) {
    // r02 stamps (gpurun_out/r2b/stamps.json): 1180 / 2080 / 2590 / 1530 cycles per tile for layer_0 / 256x256 / layer_5 / head;
    // head swept 100..200 (1.40 / 1.20 / 1.13 / 1.12 ms per fine launch at 100 / 130 / 160 / 200)
    // layer_1 recomputes h0 (wgrad_l1_recompute, 20 KiB tiles but 22 MFMAs and an LDS exchange per tile): swept 160 / 204 / 240 /
    // 280 -> 1.27 / 1.08 / 1.056 / 1.064 ms per fine launch
    // layer_7 recomputes dz7 (wgrad_l7_recompute, 18 KiB tiles): 204 -> 240; with the copies issued behind the first half's MFMAs
    // the plain jobs gained most, tools/tune_costs.py (coordinate search on the box) moved the others up: coarse + fine launch
    // 1.439 -> 1.382 ms
    // (the defaults are set per job KIND at creation, default_wgrad_cost: 128 first layer, 264 layer_1, 204 plain, 267 concat, 240
    // last layer, 193 head -- i.e. 128, 264, 204, 204, 204, 267, 204, 240, 193 for the default shape)
    int total = 0;
    for (int j = 0; j < n_jobs; ++j) total += cost[j] > 0 ? cost[j] : 0;
    std::vector<int32_t> plan;
    job_wg0.assign(n_jobs + 1, 0);
    for (int j = 0; j < n_jobs; ++j) {
        job_wg0[j] = (int32_t)plan.size() / 4;
        if (cost[j] <= 0) continue;          // a sweep may switch a job off (its gradient is then missing: timing experiments only)
        int ns = (cost[j] * (n_wg - 4) + total / 2) / total; if (ns < 1) ns = 1;
        for (int s = 0; s < ns; ++s) { plan.push_back(j); plan.push_back(s); plan.push_back(ns); plan.push_back(0); }
    }
    job_wg0[n_jobs] = (int32_t)plan.size() / 4;
    return plan;
}
int default_wgrad_cost(int kind) { const int c[6] = {128, 264, 204, 267, 240, 193}; return c[kind >= 0 && kind < 6 ? kind : 2]; }

}  // namespace

namespace {

int fail(knerf_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(ctx, KNERF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

size_t stream_bytes(int blocks) { return (size_t)((blocks + kPageBlocks - 1) / kPageBlocks * kPageBlocks + kTailPages * kPageBlocks) * 1024; }

// compose = false: the caller has already composed the heads of both nets in one launch (knerf_apply_adam)
int repack(knerf_ctx* ctx, int n, hipStream_t s, bool compose = true) {
    Net& N = ctx->net[n];
    if (ctx->generic) {
        HIPCHK(gen::pack_weights(ctx->gplan, N.w, ctx->gnet[n], s));
        return KNERF_OK;
    }
    if (compose) HIPCHK(launch_head_compose(N.w, nullptr, ctx->si.trunk_params, ctx->si.units, ctx->si.trunk_x, ctx->si.trunk_x_slots, ctx->si.dir_dim, ctx->si.dir_slots, s));   // the composed head behind the parameters (layout.h), then the bf16 streams
    HIPCHK(launch_pack(N.w, ctx->tab.d_fwd, reinterpret_cast<unsigned short*>(N.fwd_stream.get()), (size_t)ctx->si.fwd_blocks * 512, s));
    HIPCHK(launch_pack(N.w, ctx->tab.d_bwd, reinterpret_cast<unsigned short*>(N.bwd_stream.get()), (size_t)ctx->si.bwd_blocks * 512, s));
    HIPCHK(launch_gather_f32(N.w, ctx->tab.d_bias, N.bias, (size_t)ctx->si.fwd_bias_tiles * 32, s));
    return KNERF_OK;
}

size_t tiles_for(long long n_samples) {
    size_t t = (size_t)((n_samples + kTile - 1) / kTile);
    constexpr size_t q = kWaves > kSavedGroup ? kWaves : kSavedGroup;
    return (t + q - 1) / q * q;                  // whole workgroups (and whole layout groups, layout.h)
}

// a host table -> a device buffer of exactly its size
hipError_t upload(DevBuf<int>& b, const std::vector<int32_t>& v) {
    b.reset();
    if (hipError_t e = b.grow(v.size(), nullptr)) return e;
    return hipMemcpy(b, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice);
}

// (re)build the wgrad plan from ctx->wgrad_cost and upload it with the jobs' workgroup offsets
int upload_plan(knerf_ctx* ctx) {
    std::vector<int32_t> job_wg0;
    std::vector<int32_t> plan = build_wgrad_plan(ctx->n_cu, ctx->wgrad_cost, ctx->si.n_jobs, job_wg0);
    HIPCHK(upload(ctx->tab.d_plan, plan));
    HIPCHK(upload(ctx->d_job_wg0, job_wg0));
    ctx->tab.n_plan = (int)plan.size() / 4;
    ctx->plan_dirty = false;
    return KNERF_OK;
}

// option "workspace_limit_gb": the out-of-memory paths of the callers (a merged launch or a wgrad group that does not fit) are taken
// by a REAL failed hipMalloc -- same error code, same state of the runtime's last-error word -- without filling 288 GB first
int over_limit(knerf_ctx* ctx, double bytes) {
    if (ctx->ws_limit_gb <= 0 || bytes <= ctx->ws_limit_gb * 1e9) return KNERF_OK;
    void* never = nullptr;
    HIPCHK(hipMalloc(&never, (size_t)1 << 50));
    (void)hipFree(never);
    return KNERF_OK;
}

// the occupancy compaction workspace of a pass of n samples (fused path): ballots [ceil(n / 64)] u64, list [n], per-workgroup counts and
// offsets [occ_blocks(n)] each, the list's length
struct OccWs { unsigned long long* masks; int *list, *blk_cnt, *blk_off, *count; };
size_t occ_ws_bytes(long long n) { return (size_t)((n + 63) / 64) * 8 + (size_t)n * 4 + (size_t)occ_blocks(n) * 8 + 4; }
OccWs occ_ws_view(char* base, long long n) {
    OccWs w;
    w.masks = reinterpret_cast<unsigned long long*>(base);
    w.list = reinterpret_cast<int*>(base + (size_t)((n + 63) / 64) * 8);
    w.blk_cnt = w.list + n;
    w.blk_off = w.blk_cnt + occ_blocks(n);
    w.count = w.blk_off + occ_blocks(n);
    return w;
}
bool occ_attached(const knerf_ctx* ctx) { return ctx->occ[0].grid.bits || ctx->occ[1].grid.bits; }

// early ray termination (options "termination_threshold" / "termination_segment"): the segment length of a pass of S samples (a
// segment longer than the pass is the whole pass), and the fused path's workspace of a pass of R rays: ballots [term_blocks * 32]
// u64, T [R], the segment's list [R * L], per-workgroup counts / offsets, the list's length
int term_segment(const knerf_ctx* ctx, int S) { return ctx->term_L < S ? ctx->term_L : S; }
struct TermWs { unsigned long long* masks; float* T; int *list, *blk_cnt, *blk_off, *count; };
size_t term_ws_bytes(long long R, int L) { return (size_t)term_blocks(R, L) * (kTermWords * 8 + 8) + (size_t)R * 4 + (size_t)R * L * 4 + 4; }
TermWs term_ws_view(char* base, long long R, int L) {
    TermWs w;
    const long long nb = term_blocks(R, L);
    w.masks = reinterpret_cast<unsigned long long*>(base);
    w.T = reinterpret_cast<float*>(base + (size_t)nb * kTermWords * 8);
    w.list = reinterpret_cast<int*>(w.T + R);
    w.blk_cnt = w.list + R * L;
    w.blk_off = w.blk_cnt + nb;
    w.count = w.blk_off + nb;
    return w;
}
// training behind the grids (option "occupancy_train"): for one net / for either net
bool occ_train_on(const knerf_ctx* ctx, int net) { return ctx->occ_train && ctx->occ[net].grid.bits; }
bool occ_train_any(const knerf_ctx* ctx) { return ctx->occ_train && occ_attached(ctx); }

// the view of the general-shape path's buffers that generic.hip takes
gen::Workspace gen_view(const GenWsBufs& b, size_t mp) { return gen::Workspace{mp, b.act, b.dz, b.mask, b.zc}; }

// Every buffer size of passes of up to R rays, as element counts of the buffers' own types: the one place that knows them (pure host
// arithmetic on the configuration).  Training buffers of the fused path hold `group` coarse-pass regions followed by one fine-pass
// region, so that one weight-gradient launch covers the coarse passes of a group of chunks (launch_wgrad_tiles below); group 1: the
// coarse and the fine pass of a chunk share one region (each pass's weight gradients follow it at once).
struct WsSizes {
    size_t raw, w_c, t_f, img_tmp;             // inference buffers
    size_t tiles_c, tiles;                     // sample tiles of one coarse region / of all regions of the training workspaces
    size_t draw, loss_partial;                 // loss_partial: the loss, then the objective's four terms (composite_ext.h)
    size_t act, mask, dz, tile_list_g;         // fused path: saved regions (bytes); the list of a group of coarse passes (group > 1)
    size_t mp, g_act, g_zc, g_dz, g_mask;      // general-shape path (generic.h): padded rows and its forward / training buffers
    size_t occ_ws, occ_c;                      // compaction workspace; each of the compacted raw and dL/draw
    size_t term_ws;                            // the largest of the coarse and the fine pass's needs
    // (tile_flags and tile_list hold `tiles` ints each)
    double base_bytes(bool generic) const { return 4.0 * (raw + w_c + t_f + img_tmp) + (generic ? 2.0 * g_act + 4.0 * g_zc : 0.0); }
    double train_bytes(bool generic) const {
        return 4.0 * (draw + loss_partial + 2 * tiles) + (generic ? 2.0 * g_dz + (double)g_mask : (double)act + mask + dz + 4.0 * tile_list_g);
    }
};
WsSizes ws_sizes(const knerf_ctx* ctx, int R, int group = 1) {
    const size_t Nc = (size_t)ctx->cfg.n_coarse, Na = Nc + ctx->cfg.n_fine, ns = (size_t)R * Na;
    WsSizes z{};
    z.raw = ns * 4; z.w_c = (size_t)R * Nc; z.t_f = ns; z.img_tmp = (size_t)R * 8;
    z.tiles_c = tiles_for((long long)((size_t)R * Nc));
    z.tiles = group == 1 ? tiles_for((long long)ns) : (size_t)group * z.tiles_c + tiles_for((long long)ns);
    z.draw = ns * 4; z.loss_partial = 5 * (((size_t)R + 3) / 4);
    if (ctx->generic) {
        z.mp = gen::padded_rows((long long)ns);
        z.g_act = ctx->gplan.act_elems_per_row * z.mp; z.g_zc = z.mp * 32;
        z.g_dz = ctx->gplan.dz_elems_per_row * z.mp; z.g_mask = gen::relu_bits_bytes(ctx->gplan, z.mp);
    } else {
        z.act = saved_region_bytes(z.tiles, ctx->si.act_blocks); z.mask = saved_region_bytes(z.tiles, ctx->si.mask_blocks);
        z.dz = saved_region_bytes(z.tiles, ctx->si.dz_blocks);
        z.tile_list_g = group > 1 ? (size_t)group * z.tiles_c : 0;
    }
    z.occ_ws = occ_ws_bytes((long long)ns); z.occ_c = ns * 4;
    const size_t tc = term_ws_bytes(R, term_segment(ctx, (int)Nc)), tf = term_ws_bytes(R, term_segment(ctx, (int)Na));
    z.term_ws = tc > tf ? tc : tf;
    return z;
}

// grow-only workspaces; the zero-fills are enqueued on the caller's stream `s`, the one the consuming kernels run on
// (hipMalloc / hipFree themselves synchronise the device).
// Inference buffers (raw, w_c, t_f, img_tmp) follow the largest chunk of ANY call; the training workspaces of the fused path
// (draw, act / mask / dz, tile flags and lists) follow the largest TRAINING chunk and group, so that a render with a larger
// ray_chunks never re-sizes the training regions.  The general-shape path keeps one size for everything (its activations are forward
// buffers too).  Each group of buffers gives its memory back before it is allocated again, and its policy counter (ws_rays, ws_train,
// ws_occ_rays, ...) reads 0 until every buffer of the group is there: after a failed allocation the next call re-sizes the whole group.
int ensure_ws_impl(knerf_ctx* ctx, int n_rays, bool train, hipStream_t s, int group) {
    const bool generic = ctx->generic;
    bool grow_base, grow_train, grow_occ = false, grow_occ_train = false, grow_term = false;
    int R = n_rays > ctx->ws_train_rays ? n_rays : ctx->ws_train_rays;          // the training buffers' size
    if (generic) {
        if (n_rays <= ctx->ws_rays && (!train || ctx->ws_train)) return KNERF_OK;
        R = n_rays = n_rays > ctx->ws_rays ? n_rays : ctx->ws_rays;
        grow_base = true; grow_train = train || ctx->ws_train; group = 1;
    } else {
        grow_base = n_rays > ctx->ws_rays;
        grow_train = train && (!ctx->ws_train || n_rays > ctx->ws_train_rays || group > ctx->ws_group);
        // renders behind an occupancy grid: the compaction workspace (4 B + 1 bit per sample), only while a grid is attached; training
        // behind one ("occupancy_train"): the same at the training size, and the compacted raw / dL/draw (32 B per sample)
        const bool occ_tr = train && occ_train_any(ctx);
        grow_occ = (train ? occ_tr : occ_attached(ctx)) && n_rays > ctx->ws_occ_rays;
        grow_occ_train = occ_tr && n_rays > ctx->ws_occ_train_rays;
    }
    const WsSizes z = ws_sizes(ctx, n_rays), zt = ws_sizes(ctx, R, group);
    // renders with early ray termination ("termination_threshold" > 0): T, the segment's ballots, counts and list (about 4 L + 8 bytes per ray)
    if (!generic) grow_term = !train && ctx->term_eps > 0 && z.term_ws > ctx->term_ws.size();
    if (!grow_base && !grow_train && !grow_occ && !grow_occ_train && !grow_term) return KNERF_OK;
    // the sum of what is about to be requested (tile flags, tile lists and loss partials included; the general-shape path no longer
    // counts the head buffer it used to allocate without reading it)
    if (int r = over_limit(ctx, (grow_base ? z.base_bytes(generic) : 0.0) + (grow_train ? zt.train_bytes(generic) : 0.0) + (grow_occ ? (double)z.occ_ws : 0.0) +
                                    (grow_occ_train ? 8.0 * z.occ_c : 0.0) + (grow_term ? (double)z.term_ws : 0.0))) return r;
    HIPCHK(hipStreamSynchronize(s));               // nothing enqueued earlier may still use the buffers that are freed below
    if (grow_base) {
        release(ctx->raw, ctx->w_c, ctx->t_f, ctx->img_tmp, ctx->gws_buf.act, ctx->gws_buf.zc);
        if (generic) release(ctx->draw, ctx->gws_buf.dz, ctx->gws_buf.mask);      // one size for everything: these follow below
        ctx->ws_rays = 0; ctx->gws = gen::Workspace{};
        HIPCHK(ctx->raw.grow(z.raw, s));
        HIPCHK(ctx->w_c.grow(z.w_c, s));
        HIPCHK(ctx->t_f.grow(z.t_f, s));
        HIPCHK(ctx->img_tmp.grow(z.img_tmp, s));
        if (generic) {
            HIPCHK(ctx->gws_buf.act.grow(z.g_act, s, true));
            HIPCHK(ctx->gws_buf.zc.grow(z.g_zc, s));
            ctx->gws = gen_view(ctx->gws_buf, z.mp);
        }
        ctx->ws_rays = n_rays;
    }
    if (grow_occ) {
        ctx->ws_occ_rays = 0;
        release(ctx->occ_ws);
        HIPCHK(ctx->occ_ws.grow(z.occ_ws, s));
        ctx->ws_occ_rays = n_rays;
    }
    if (grow_term) HIPCHK(ctx->term_ws.grow(z.term_ws, s));
    if (grow_occ_train) {
        ctx->ws_occ_train_rays = 0;
        release(ctx->occ_raw_c, ctx->occ_draw_c);
        HIPCHK(ctx->occ_raw_c.grow(z.occ_c, s));
        HIPCHK(ctx->occ_draw_c.grow(z.occ_c, s));
        ctx->ws_occ_train_rays = n_rays;
    }
    if (grow_train) {
        release(ctx->draw, ctx->act, ctx->mask, ctx->dz, ctx->gws_buf.dz, ctx->gws_buf.mask);
        release(ctx->tile_flags, ctx->tile_list, ctx->tile_list_g, ctx->loss_partial);
        ctx->ws_train = false; ctx->ws_train_rays = 0; ctx->ws_group = 1; ctx->group_cache = 0;
        HIPCHK(ctx->draw.grow(zt.draw, s));
        if (generic) {
            HIPCHK(ctx->gws_buf.dz.grow(zt.g_dz, s, true));
            HIPCHK(ctx->gws_buf.mask.grow(zt.g_mask, s));
        } else {
            HIPCHK(ctx->act.grow(zt.act, s, true));
            HIPCHK(ctx->mask.grow(zt.mask, s));
            HIPCHK(ctx->dz.grow(zt.dz, s, true));                     // block kDzHead+1 is never written and must read 0
        }
        // dead-tile skipping: per-tile flags (deterministic mode) and the list of live tiles of the current pass
        HIPCHK(ctx->tile_flags.grow(zt.tiles, s, true));
        HIPCHK(ctx->tile_list.grow(zt.tiles, s));
        HIPCHK(ctx->tile_list_g.grow(zt.tile_list_g, s));
        HIPCHK(ctx->loss_partial.grow(zt.loss_partial, s));
        if (generic) ctx->gws = gen_view(ctx->gws_buf, zt.mp);
        ctx->ws_train = true; ctx->ws_train_rays = R; ctx->ws_group = group;
    }
    return KNERF_OK;
}

// A failed hipMalloc stays behind as the runtime's LAST ERROR: every launch helper ends in `return hipGetLastError()`, so the first
// kernel after a failed allocation would report hipErrorOutOfMemory although the caller's retry at a smaller size succeeded
// (ADVICE r05).  The word is read -- which clears it -- here, where the failure is already on its way to the caller as a status.
int ensure_ws(knerf_ctx* ctx, int n_rays, bool train, hipStream_t s, int group = 1) {
    const int r = ensure_ws_impl(ctx, n_rays, train, s, group);
    if (r) (void)hipGetLastError();
    return r;
}

// kernel classes reported by knerf_profile_read
enum ProfId { P_FWD_C = 0, P_FWD_F, P_COMPOSITE, P_SAMPLE, P_BWD_C, P_BWD_F, P_WGRAD_C, P_WGRAD_F, P_ADAM, P_COUNT };

struct ProfScope {
    knerf_ctx* c; hipStream_t s; int idx = -1;
    ProfScope(knerf_ctx* ctx, hipStream_t st, int id) : c(ctx), s(st) {
        if (!c->prof_on) return;
        knerf_ctx::ProfRec r{id, nullptr, nullptr};
        if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return;
        (void)hipEventRecord(r.e0, s);
        c->prof.push_back(r); idx = (int)c->prof.size() - 1;
    }
    ~ProfScope() { if (idx >= 0) (void)hipEventRecord(c->prof[idx].e1, s); }
};

// a context created with KNERF_FLAG_ENCODED_WIDTHS is a stand-alone NeRFMLP: it has no ray encodings, samplers or workspaces
int check_rays(knerf_ctx* ctx, const char* what) {
    if (!ctx) return KNERF_ERR_INVALID;
    if (ctx->mlp_only) return fail(ctx, KNERF_ERR_INVALID, std::string(what) + ": this context was created with KNERF_FLAG_ENCODED_WIDTHS (NeRFMLP.__call__ only)");
    return KNERF_OK;
}

int check_net(knerf_ctx* ctx, int net) {
    if (!ctx) return KNERF_ERR_INVALID;
    if (net != KNERF_COARSE && net != KNERF_FINE) return fail(ctx, KNERF_ERR_INVALID, "net must be 0 (coarse) or 1 (fine)");
    return KNERF_OK;
}

// dead-tile skipping applies when 32-sample tiles do not straddle rays in either pass (both MLP paths since round 5: the
// general-shape kernels walk the same list of live tiles, generic.hip)
bool skipping(const knerf_ctx* ctx) {
    return ctx->skip_dead && ctx->cfg.n_coarse % kTile == 0 && (ctx->cfg.n_coarse + ctx->cfg.n_fine) % kTile == 0;
}

// A fresh (zero) counter for one list of live tiles.  The ring is zeroed by one memset when a call takes its first counter, and again
// if a call runs through the whole ring (the consumers of its earlier counters are enqueued by then; the stream orders the memset).
int next_tile_counter(knerf_ctx* ctx, hipStream_t s, int** count) {
    if (ctx->tile_counter_next >= (int)ctx->tile_count.size()) ctx->tile_counter_next = 0;     // not reached by the entry points: they size the ring first
    if (ctx->tile_counter_next == 0) HIPCHK(hipMemsetAsync(ctx->tile_count, 0, ctx->tile_count.bytes(), s));
    *count = ctx->tile_count + ctx->tile_counter_next++;
    return KNERF_OK;
}

// The ring holds every counter one call takes (grow-only): a wrap inside a call would zero a group's counter that later coarse
// passes still append to, and the grouped weight-gradient launch would then see a short list.
int ensure_tile_counters(knerf_ctx* ctx, hipStream_t s, long long need) {
    if (need <= (long long)ctx->tile_count.size()) return KNERF_OK;
    long long n = knerf_ctx::kTileCounters;
    while (n < need) n *= 2;
    HIPCHK(ctx->tile_count.grow((size_t)n, s));    // (behind a synchronise: consumers of the old ring's counters have finished)
    ctx->tile_counter_next = 0;
    return KNERF_OK;
}

// Deterministic mode: tile flags -> ASCENDING list (its per-workgroup ranges need the order) by the one-workgroup compaction kernel.
int compact_tiles(knerf_ctx* ctx, hipStream_t s, const int* flags, int n, int period, int real, int* list, int** count) {
    if (int r = next_tile_counter(ctx, s, count)) return r;
    HIPCHK(launch_compact_tiles(flags, n, period, real, list, *count, nullptr, s));
    return KNERF_OK;
}

// weight gradients of `net` over n_tiles sample tiles starting at tile `tile0` of the act / mask / dz workspaces.  live: null, or the
// list of live tiles (indices relative to tile0) with its device counter.
int launch_wgrad_tiles(knerf_ctx* ctx, hipStream_t s, int net, size_t tile0, size_t n_tiles, const int* live, const int* live_count) {
    WgradArgs wa{};
    wa.act = ctx->act + saved_tile_off(tile0, ctx->si.act_blocks); wa.dz = ctx->dz + saved_tile_off(tile0, ctx->si.dz_blocks);
    wa.mask = ctx->mask + saved_tile_off(tile0, ctx->si.mask_blocks);
    wa.shape = ctx->shape; wa.n_jobs = ctx->si.n_jobs; wa.aux_base = ctx->si.param_count;
    wa.grad = ctx->net[net].g; wa.aux = ctx->net[net].aux; wa.dst = ctx->tab.d_wgrad;
    wa.fwd_stream = ctx->net[net].fwd_stream; wa.bias = ctx->net[net].bias; wa.bwd_stream = ctx->net[net].bwd_stream;
    wa.n_tiles = (long long)n_tiles;
    wa.plan = ctx->tab.d_plan; wa.n_plan = ctx->tab.n_plan; wa.net = net;
    for (int j = 0; j <= ctx->si.n_jobs; ++j) wa.job_off[j] = ctx->tab.wgrad_off[j];
    if (live) { wa.live = live; wa.n_live = live_count; wa.by_range = ctx->deterministic ? 1 : 0; }
    wa.stats = ctx->tile_stats + 4 * net;
    if (ctx->deterministic) {
        // per-workgroup slabs (zeroed: a workgroup without tiles writes nothing) + the ordered second pass
        const size_t slabs = wgrad_partial_floats(ctx->tab.n_plan, ctx->si.partial_stride);
        HIPCHK(ctx->partial.grow(slabs, s));
        HIPCHK(hipMemsetAsync(ctx->partial, 0, slabs * sizeof(float), s));
        wa.partial = ctx->partial;
    }
    ProfScope ps(ctx, s, P_WGRAD_C + net);
    HIPCHK(launch_wgrad(wa, s));
    if (ctx->deterministic) HIPCHK(launch_wgrad_reduce(wa, ctx->d_job_wg0, ctx->si.partial_stride, s));
    return KNERF_OK;
}

// One pass of one net over R rays of S samples.  target set: a training pass (loss, dL/draw, dgrad and, with wgrad_now, its weight gradients).
static_assert(KNERF_COARSE == 0 && KNERF_FINE == 1 && P_FWD_F == P_FWD_C + 1 && P_BWD_F == P_BWD_C + 1 && P_WGRAD_F == P_WGRAD_C + 1,
              "the net is the index of its stats words, objective bit and profile class");
struct Pass {
    int net;
    const float *o, *d, *t;                 // [R,3], [R,3], [R,S]
    int R, S;
    float *image = nullptr, *depth = nullptr, *weights = nullptr;
    const float* target = nullptr;
    float inv_chunks = 1.f;
    float* loss = nullptr;
    size_t tile0 = 0;                       // first tile of this pass in the training workspaces
    bool wgrad_now = true;                  // false: the caller launches the weight gradients later over several passes (launch_wgrad_tiles)
    // (default-mode skipping, coarse pass of a grouped launch) the group's counter: the pass's live tiles are appended to
    // ctx->tile_list_g as well, as indices relative to the group's first region (+ tile0)
    int* group_count = nullptr;
    // a pass of knerf_render_chunk -- the net's occupancy grid, if one is attached, applies; to training passes only under option
    // "occupancy_train" (never to forward_chunk or queries)
    bool render = false;
};

// the lists of a compaction workspace (OccWs / TermWs) as the mark kernels take them
template <class Args, class Ws>
void take_lists(Args& a, const Ws& w) { a.masks = w.masks; a.blk_cnt = w.blk_cnt; a.blk_off = w.blk_off; a.list = w.list; a.count = w.count; }

// the fused MLP on a list of live samples of the pass (query.hip list mode); the caller sets n
QueryArgs list_query(const knerf_ctx* ctx, const Pass& p, const int* list, const int* count) {
    QueryArgs q{};
    q.stream = ctx->net[p.net].fwd_stream; q.bias = ctx->net[p.net].bias; q.shape = ctx->shape;
    q.raw = ctx->raw; q.list = list; q.count = count; q.o = p.o; q.d = p.d; q.t = p.t; q.S = p.S;
    return q;
}

int run_pass(knerf_ctx* ctx, hipStream_t s, const Pass& p) {
    const int net = p.net, R = p.R, S = p.S;
    const float *o = p.o, *d = p.d, *t = p.t;
    const size_t tile0 = p.tile0;
    const bool train = p.target != nullptr;
    const OccGrid* og = ((p.render && !train) || (train && occ_train_on(ctx, net))) && ctx->occ[net].grid.bits ? &ctx->occ[net].grid : nullptr;
    // fused training behind a grid: forward, dgrad and weight gradients on the compacted list of live samples (train_list.h)
    const bool compact = og && train && !ctx->generic;
    // early ray termination: render passes only, while "termination_threshold" > 0 (termination.h)
    const bool term = p.render && !train && ctx->term_eps > 0;
    OccArgs oa{};
    if (og) {
        oa.grid = *og;
        oa.o = o; oa.d = d; oa.t = t; oa.n = (long long)R * S; oa.S = S; oa.raw = ctx->raw;
        oa.stats = (train ? ctx->occ_train_stats : ctx->occ_stats) + 2 * net;
        if (!ctx->generic && oa.n >= (1ll << 31))       // the list holds int32 sample indices
            return fail(ctx, KNERF_ERR_INVALID, "pass behind an occupancy grid: a pass of 2^31 samples or more (use a smaller ray_chunks)");
    }
    TermArgs ta{};
    if (term) {
        if (og) { ta.grid = oa.grid; ta.has_grid = 1; ta.occ_stats = oa.stats; }
        ta.o = o; ta.d = d; ta.t = t; ta.raw = ctx->raw; ta.R = R; ta.S = S; ta.L = term_segment(ctx, S); ta.eps = (float)ctx->term_eps;
        ta.stats = ctx->term_stats + 2 * net;
        if (!ctx->generic && (long long)R * S >= (1ll << 31))       // the list holds int32 sample indices
            return fail(ctx, KNERF_ERR_INVALID, "pass with early ray termination: a pass of 2^31 samples or more (use a smaller ray_chunks)");
    }
    FwdArgs fa{};
    fa.stream = ctx->net[net].fwd_stream; fa.bias = ctx->net[net].bias;
    fa.o = o; fa.d = d; fa.t = t; fa.raw = ctx->raw;
    fa.act = ctx->act ? ctx->act + saved_tile_off(tile0, ctx->si.act_blocks) : nullptr;
    fa.mask = ctx->mask ? ctx->mask + saved_tile_off(tile0, ctx->si.mask_blocks) : nullptr;
    fa.n_samples = (long long)R * S; fa.S = S; fa.net = net; fa.shape = ctx->shape;
    {
        ProfScope ps(ctx, s, P_FWD_C + net);
        if (ctx->generic) {
            HIPCHK(gen::forward(ctx->gplan, ctx->gws, ctx->gnet[net], ctx->net[net].w, o, d, t, fa.n_samples, S, ctx->raw, s));
            // general-shape path: the MLP ran on every sample; the dead ones are zeroed behind it (same outputs, no speed-up)
            if (og) HIPCHK(launch_occupancy_mark(oa, s));
            // ... and the terminated ones behind the dead ones, by the same cut rule
            if (term) HIPCHK(launch_termination_walk(ta, s));
        } else if (compact) {
            // fused training: ordered compaction of the live samples, then the SAVE forward on the list alone; saved tensors of compacted
            // tile i / 32, raw to raw[list[i]]
            take_lists(oa, occ_ws_view(ctx->occ_ws, oa.n));
            HIPCHK(launch_occupancy_mark(oa, s));
            TrainListArgs la{};
            la.f = fa; la.list = oa.list; la.count = oa.count;
            HIPCHK(launch_mlp_fwd_list(la, s));
        } else if (term) {
            // fused path with early ray termination: one round per segment -- fold the previous segment into T, cut, grid, ordered
            // compaction of the segment's live samples -- then the fused MLP on that list; no host synchronisation between rounds
            const TermWs w = term_ws_view(ctx->term_ws, R, ta.L);
            ta.T = w.T; take_lists(ta, w);
            QueryArgs q = list_query(ctx, p, w.list, w.count);
            for (int k = 0; k * ta.L < S; ++k) {
                ta.k = k;
                HIPCHK(launch_termination_round(ta, s));
                const int Lk = S - k * ta.L < ta.L ? S - k * ta.L : ta.L;
                q.n = (long long)R * Lk;
                HIPCHK(launch_query_list(q, s));
            }
        } else if (og) {
            // fused path: ordered compaction of the live samples, then the fused MLP on the list alone (query.hip list mode)
            take_lists(oa, occ_ws_view(ctx->occ_ws, oa.n));
            HIPCHK(launch_occupancy_mark(oa, s));
            QueryArgs q = list_query(ctx, p, oa.list, oa.count);
            q.n = oa.n;
            HIPCHK(launch_query_list(q, s));
        } else {
            HIPCHK(launch_mlp_fwd(fa, train, s));
        }
    }
    CompositeArgs ca{};
    ca.raw = ctx->raw; ca.t = t; ca.target = p.target; ca.image = p.image; ca.depth = p.depth; ca.weights = p.weights;
    ca.draw = train ? ctx->draw.get() : nullptr; ca.loss = p.loss; ca.R = R; ca.S = S; ca.white = ctx->cfg.white_background;
    ca.grad_scale = 2.0f / (3.0f * (float)R) * p.inv_chunks;
    ca.loss_scale = p.inv_chunks / (3.0f * (float)R);
    // (the compacted path makes its own list of live tiles behind compositing, below)
    const bool skip = train && skipping(ctx) && !compact;
    const size_t n_tiles = tiles_for(fa.n_samples);
    long long* const tile_stats = ctx->tile_stats + 4 * net;
    int* live_count = nullptr;
    if (skip && ctx->deterministic) {
        ca.tile_flags = ctx->tile_flags + tile0;                     // flags now, an ascending list from the compaction kernel below
    } else if (skip) {
        if (int r = next_tile_counter(ctx, s, &live_count)) return r;     // the compositing kernel appends the live tiles itself
        ca.tile_list = ctx->tile_list; ca.tile_count = live_count;
        if (p.group_count) { ca.tile_list2 = ctx->tile_list_g; ca.tile_count2 = p.group_count; ca.tile_off2 = (int)tile0; }
    }
    if (train && ctx->deterministic) ca.loss_partial = ctx->loss_partial;
    // an extended objective (knerf_set_objective): the launch goes to composite_ext.hip; the plain objective never does
    CompositeExt ce{};
    const bool ext = train && ctx->obj_ext;
    if (ext) {
        const bool regs = (ctx->obj.nets >> net) & 1;
        ce.loss_kind = ctx->obj.loss_kind; ce.huber_delta = ctx->obj.huber_delta;
        ce.lambda_d = regs ? ctx->obj.distortion : 0.f; ce.lambda_e = regs ? ctx->obj.opacity_entropy : 0.f;
        ce.reg_scale = p.inv_chunks / (float)R;
        ce.terms = ctx->d_terms + 4 * net;
        if (ca.loss_partial) ce.terms_partial = ctx->loss_partial + ((size_t)ctx->ws_train_rays + 3) / 4;
    }
    {
        ProfScope ps(ctx, s, P_COMPOSITE);
        HIPCHK(launch_composite(ca, ext ? &ce : nullptr, s));
        if (ca.loss_partial) HIPCHK(launch_loss_reduce(ca.loss_partial, (R + 3) / 4, p.loss, s));
        if (ce.terms_partial) HIPCHK(launch_terms_reduce(ce.terms_partial, (R + 3) / 4, ce.terms, s));
        // deterministic mode: the pass's live tiles (indices relative to tile0) in ascending order; the padding tiles behind the
        // last real one count as dead
        if (ca.tile_flags) { if (int r = compact_tiles(ctx, s, ca.tile_flags, (int)n_tiles, (int)n_tiles, (int)(fa.n_samples / kTile), ctx->tile_list, &live_count)) return r; }
        if (compact) {
            // raw and dL/draw of the live samples in list order (the last tile padded with zeros), one flag per compacted tile, then the ascending
            // list of the flagged tiles -- in both modes.  Compacted tiles straddle rays, so the per-ray tile flags of compositing (which
            // need S % 32 == 0) do not apply; the flags come from the gathered dL/draw instead, with the same dead-sample rule.
            HIPCHK(launch_occupancy_train_gather(oa.list, oa.count, ctx->raw, ctx->draw, ctx->occ_draw_c, ctx->occ_raw_c, ctx->tile_flags + tile0, fa.n_samples,
                                                 (long long)n_tiles, ctx->skip_dead ? 1 : 0, s));
            if (int r = compact_tiles(ctx, s, ctx->tile_flags + tile0, (int)n_tiles, (int)n_tiles, (int)n_tiles, ctx->tile_list, &live_count)) return r;
        }
    }
    if (train && ctx->generic) {
        ProfScope ps(ctx, s, P_BWD_C + net);
        if (og) {              // general-shape path behind a grid: no gradient from the dead samples (the mark kernel zeroes dL/draw there)
            OccArgs od = oa;
            od.raw = ctx->draw; od.stats = nullptr;
            HIPCHK(launch_occupancy_mark(od, s));
        }
        // general-shape path: the slab arena of generic.hip (the fused path's lives in launch_wgrad_tiles)
        if (ctx->deterministic) HIPCHK(ctx->partial.grow(gen::wgrad_partial_floats(ctx->gplan), s));
        HIPCHK(gen::backward(ctx->gplan, ctx->gws, ctx->gnet[net], ctx->raw, ctx->draw, fa.n_samples, ctx->net[net].g, s,
                             ctx->deterministic ? ctx->partial.get() : nullptr, skip ? ctx->tile_list.get() : nullptr, skip ? live_count : nullptr,
                             skip ? tile_stats : nullptr));
    } else if (train) {
        BwdArgs ba{};
        ba.stream = ctx->net[net].bwd_stream; ba.raw = ctx->raw; ba.draw = ctx->draw; ba.mask = fa.mask; ba.dz = ctx->dz + saved_tile_off(tile0, ctx->si.dz_blocks);
        ba.n_samples = fa.n_samples; ba.net = net; ba.shape = ctx->shape;
        if (skip) { ba.live = ctx->tile_list; ba.n_live = live_count; ba.stats = tile_stats; }
        if (compact) {
            ba.raw = ctx->occ_raw_c; ba.draw = ctx->occ_draw_c; ba.live = ctx->tile_list; ba.n_live = live_count;
            ba.stats = ctx->skip_dead ? tile_stats : nullptr;
        }
        { ProfScope ps(ctx, s, P_BWD_C + net); HIPCHK(launch_mlp_bwd(ba, s)); }
        if (p.wgrad_now) { if (int r = launch_wgrad_tiles(ctx, s, net, tile0, n_tiles, skip || compact ? ctx->tile_list.get() : nullptr, live_count)) return r; }
    }
    return KNERF_OK;
}

// the wgrad head jobs leave sums in ctx->aux; this turns them into the gradients of features / rgb_features / rgb of both
// nets (optim.hip head_expand).  Linear in the sums, so once per batch of chunks is the same as once per chunk.
int expand_head_grads(knerf_ctx* ctx, hipStream_t s) {
    if (ctx->generic) {
        for (int n = 0; n < 2; ++n) HIPCHK(gen::expand_head(ctx->gplan, ctx->gnet[n], ctx->net[n].w, ctx->net[n].g, s));
        return KNERF_OK;
    }
    HIPCHK(launch_head_expand(ctx->net[0].w, ctx->net[0].aux, ctx->net[0].g, ctx->net[1].w, ctx->net[1].aux, ctx->net[1].g, ctx->si.trunk_params, ctx->si.units, ctx->si.trunk_x, ctx->si.trunk_x_slots, ctx->si.dir_dim, ctx->si.dir_slots, s));
    return KNERF_OK;
}

// One chunk through both nets.  With group > 1 the chunk's COARSE pass occupies slot `slot` of the coarse regions (tiles
// [slot tc, (slot+1) tc)) and its weight gradients are left to one launch over the whole group (knerf_train_batch); the fine pass
// uses the single fine region behind them and is followed by its own wgrad launch as before.  Why only the coarse pass: a wgrad
// launch carries ~44 us of flush, ramp and tail, 12 % of a coarse launch (8192 tiles at ray_chunks 4096) but 4 % of a fine one, and
// launches of 4 x 24576 tiles ran 4.7 % SLOWER per tile (41.4 vs 39.6 ns; power-limited clocks over a 4 ms kernel) -- measured with
// both nets grouped: coarse 2.86 -> 2.57 ms, fine 7.8 -> 8.15 ms per step.
struct Chunk {
    const float *o, *d, *t, *target, *u;    // u: null, or the fine sampler's random numbers
    uint64_t seed, ray_offset;
    int n_rays;
    float inv_chunks;
    float *loss, *c_image, *f_image;        // null: the context's own scratch
    int slot = 0, group = 1;
    int* group_count = nullptr;             // Pass::group_count of the coarse pass
};
int train_chunk_impl(knerf_ctx* ctx, hipStream_t s, const Chunk& c) {
    const int Nc = ctx->cfg.n_coarse, Na = Nc + ctx->cfg.n_fine;
    float* ls = c.loss ? c.loss : ctx->loss_tmp.get();
    const size_t tc = ws_sizes(ctx, c.n_rays).tiles_c;
    Pass p{KNERF_COARSE, c.o, c.d, c.t, c.n_rays, Nc};
    p.image = c.c_image ? c.c_image : ctx->img_tmp.get(); p.weights = ctx->w_c;
    p.target = c.target; p.inv_chunks = c.inv_chunks; p.loss = ls;
    p.tile0 = c.group == 1 ? 0 : c.slot * tc; p.wgrad_now = c.group == 1; p.group_count = c.group_count;
    if (int r = run_pass(ctx, s, p)) return r;
    if (int r = knerf_sample_fine(ctx, s, c.t, ctx->w_c, c.u, c.seed, 0, c.ray_offset, c.n_rays, ctx->t_f)) return r;
    p.net = KNERF_FINE; p.t = ctx->t_f; p.S = Na;
    p.image = c.f_image ? c.f_image : ctx->img_tmp + (size_t)c.n_rays * 4; p.weights = nullptr; p.loss = ls + 1;
    p.tile0 = c.group == 1 ? 0 : c.group * tc; p.wgrad_now = true; p.group_count = nullptr;
    return run_pass(ctx, s, p);
}

// chunks per COARSE weight-gradient launch of knerf_train_batch: up to KNERF_WGRAD_GROUP_MAX (4), within the budget
// (KNERF_WGRAD_GROUP_GB, default 40; 0 = one launch per chunk) and a quarter of the free device memory
int wgrad_group_for(knerf_ctx* ctx, int n_rays, int n_chunks) {
    if (ctx->generic || n_chunks <= 1) return 1;
    if (ctx->group_cache > 0 && ctx->group_cache_rays == n_rays && ctx->group_cache_chunks == n_chunks) return ctx->group_cache;
    auto memo = [&](int g) { ctx->group_cache_rays = n_rays; ctx->group_cache_chunks = n_chunks; ctx->group_cache = g; return g; };
    const double budget = ctx->wgrad_group_gb;
    if (budget <= 0 || ctx->wgrad_group_max <= 1) return memo(1);
    const size_t tc = ws_sizes(ctx, n_rays).tiles_c;
    const double per_chunk = (double)(saved_region_bytes(tc, ctx->si.act_blocks) + saved_region_bytes(tc, ctx->si.mask_blocks) +
                                      saved_region_bytes(tc, ctx->si.dz_blocks));   // one coarse region
    size_t free_b = 0, total_b = 0;
    double avail = budget * 1e9;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const double mine = ctx->ws_train ? (double)(ctx->act.bytes() + ctx->mask.bytes() + ctx->dz.bytes()) : 0.0;   // what a re-allocation gives back
        const double cap = 0.25 * ((double)free_b + mine);
        if (cap < avail) avail = cap;
    }
    int g = (int)(avail / per_chunk);
    const int g_max = ctx->wgrad_group_max;         // default 4: coarse launches of more than ~4 x 8192 tiles gain nothing more
    if (g > g_max) g = g_max;
    if (g > n_chunks) g = n_chunks;
    if (g <= 1) return memo(1);
    const int n_groups = (n_chunks + g - 1) / g;
    return memo((n_chunks + n_groups - 1) / n_groups);      // the smallest group that needs no more launches
}

// Chunks per LAUNCH (option "merge_chunk_rays", default 4096 rays).  `ray_chunks` is the reference's memory knob (nerf.py:100,
// 332-473: a Python loop over chunks, gradients accumulated as g / C): every ray's forward, loss term and gradient contribution is
// independent of which chunk holds it -- the per-chunk mean over R rays times 1 / C is the per-launch mean over m R rays times
// m / C, the fine sampler's random numbers are keyed by the ray's index in the batch -- so m consecutive chunks run as ONE set of
// launches: rendered outputs bit-identical, accumulated gradients equal up to the order of fp32 sums.  On this device a 4,096-ray
// launch needs 8 GB of workspace; launches of 256 / 512 / 1,024 rays (the reference's train.py defaults to 1,024) fill 256 CUs
// badly: 23.7 / 18.0 / 14.3 ms per 128 x 128 image against 13.7.  m divides the chunk count (equal-sized launches).
int merge_factor(int limit_rays, int ray_chunks, int n_chunks) {
    if (limit_rays <= 0 || n_chunks <= 1) return 1;
    for (int m = n_chunks; m > 1; --m)
        if (n_chunks % m == 0 && (long long)m * ray_chunks <= limit_rays) return m;
    return 1;
}

}  // namespace

namespace {

// knerf_mlp_call's general-shape plan, packed weights and workspace (grow-only) for n rows; also the general-shape route of the
// queries (query_general below)
int ensure_call(knerf_ctx* ctx, long long n, hipStream_t s) {
    if (!ctx->call_plan_ok) {
        const knerf_config& c = ctx->cfg;
        ctx->call_plan = ctx->mlp_only ? gen::build_plan_widths(c.n_layers, c.dense_units, c.skip_layer, c.pos_emb_xyz, c.pos_emb_dir)
                                       : gen::build_plan(c.n_layers, c.dense_units, c.skip_layer, c.pos_emb_xyz, c.pos_emb_dir);
        GenNetBufs& nb = ctx->call_net_buf;
        HIPCHK(nb.packed.grow(ctx->call_plan.packed_elems, s));
        HIPCHK(nb.head.grow(gen::head_floats(ctx->call_plan), s));
        ctx->call_net.packed = nb.packed; ctx->call_net.head = nb.head;
        ctx->call_plan_ok = true;
    }
    const size_t mp = gen::padded_rows(n);
    if (mp > ctx->call_ws.mp) {
        GenWsBufs& b = ctx->call_ws_buf;
        HIPCHK(hipStreamSynchronize(s));
        release(b.act, b.zc);
        ctx->call_ws = gen::Workspace{};
        HIPCHK(b.act.grow(ctx->call_plan.act_elems_per_row * mp, s, true));
        HIPCHK(b.zc.grow(mp * 32, s));
        ctx->call_ws = gen_view(b, mp);
    }
    return KNERF_OK;
}


// The query entry points on a shape the fused kernels do not cover (or under KNERF_FLAG_FORCE_GENERIC): points and directions of a
// chunk (query.hip gather), the positional-encoding op, knerf_mlp_call's general-shape forward, raw -> the caller's outputs (query.hip
// scatter).  Chunks are sized so that the workspaces stay near 1 GB.
int query_general(knerf_ctx* ctx, hipStream_t s, int net, const QueryArgs& q0) {
    if (int r = ensure_call(ctx, 1, s)) return r;
    const gen::Plan& p = ctx->call_plan;
    const size_t row_floats = 6 + (size_t)p.xyz_dim + (size_t)p.dir_dim + 4;
    const size_t row_bytes = p.act_elems_per_row * sizeof(unsigned short) + 64 * sizeof(float) + row_floats * sizeof(float);
    long long chunk = (long long)(((size_t)1 << 30) / row_bytes) / 1024 * 1024;
    if (chunk < 1024) chunk = 1024;
    if (chunk > q0.n) chunk = q0.n;
    if (int r = ensure_call(ctx, chunk, s)) return r;
    HIPCHK(ctx->query_tmp.grow((size_t)chunk * row_floats, s));
    float* xyz = ctx->query_tmp;
    float* dir = xyz + 3 * chunk;
    float* xenc = dir + 3 * chunk;
    float* denc = xenc + (size_t)p.xyz_dim * chunk;
    float* raw = denc + (size_t)p.dir_dim * chunk;
    HIPCHK(gen::pack_weights(p, ctx->net[net].w, ctx->call_net, s));       // the weights may have changed since the last call
    for (long long off = 0; off < q0.n; off += chunk) {
        const long long m = q0.n - off < chunk ? q0.n - off : chunk;
        QueryArgs q = q0;
        q.offset = off;
        HIPCHK(launch_query_gather(q, m, xyz, dir, s));
        if (knerf_positional_encoding(s, xyz, m, ctx->cfg.pos_emb_xyz, xenc) != KNERF_OK ||
            knerf_positional_encoding(s, dir, m, ctx->cfg.pos_emb_dir, denc) != KNERF_OK)
            return fail(ctx, KNERF_ERR_HIP, "query: positional encoding failed");
        HIPCHK(gen::forward_encoded(p, ctx->call_ws, ctx->call_net, ctx->net[net].w, xenc, denc, m, raw, s));
        HIPCHK(launch_query_scatter(q, m, raw, s));
    }
    return KNERF_OK;
}

int run_query(knerf_ctx* ctx, void* stream, int net, QueryArgs& q) {
    if (!q.raw && !q.sigma && !q.rgb) return fail(ctx, KNERF_ERR_INVALID, "query: no output (raw, sigma and rgb are all NULL)");
    if (q.n <= 0 || q.n > (1ll << 38)) return fail(ctx, KNERF_ERR_INVALID, "query: need 1 <= number of points <= 2^38");
    hipStream_t s = (hipStream_t)stream;
    if (ctx->generic) return query_general(ctx, s, net, q);
    q.stream = ctx->net[net].fwd_stream; q.bias = ctx->net[net].bias; q.shape = ctx->shape;
    HIPCHK(launch_query(q, s));
    return KNERF_OK;
}

}  // namespace

extern "C" {

size_t knerf_param_count(void) { return (size_t)kParamCount; }

size_t knerf_param_count_for(const knerf_config* cfg) {
    if (!cfg || cfg->n_layers < 1 || cfg->dense_units < 2 || cfg->skip_layer < 1 || cfg->pos_emb_xyz < 0 || cfg->pos_emb_dir < 0) return 0;
    if (cfg->flags & KNERF_FLAG_ENCODED_WIDTHS) {
        if (cfg->pos_emb_xyz < 1 || cfg->pos_emb_dir < 1) return 0;
        return (size_t)gen::build_plan_widths(cfg->n_layers, cfg->dense_units, cfg->skip_layer, cfg->pos_emb_xyz, cfg->pos_emb_dir).n_params;
    }
    return (size_t)gen::param_count(cfg->n_layers, cfg->dense_units, cfg->skip_layer, cfg->pos_emb_xyz, cfg->pos_emb_dir);
}

const char* knerf_last_error(const knerf_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int knerf_create(const knerf_config* cfg, knerf_ctx** out) {
    knerf_ctx* ctx = nullptr;
    if (!cfg || !out) return fail(nullptr, KNERF_ERR_INVALID, "null argument");
    const bool widths = (cfg->flags & KNERF_FLAG_ENCODED_WIDTHS) != 0;      // stand-alone NeRFMLP: pos_emb_* ARE the two input widths
    if (cfg->n_layers < 1 || cfg->n_layers > 64 || cfg->dense_units < 2 || cfg->dense_units > 4096 || cfg->skip_layer < 1)
        return fail(nullptr, KNERF_ERR_INVALID, "need 1 <= n_layers <= 64, 2 <= dense_units <= 4096, skip_layer >= 1");
    if (widths && (cfg->pos_emb_xyz < 1 || cfg->pos_emb_xyz > 4096 || cfg->pos_emb_dir < 1 || cfg->pos_emb_dir > 4096))
        return fail(nullptr, KNERF_ERR_INVALID, "KNERF_FLAG_ENCODED_WIDTHS: need 1 <= input width <= 4096 in pos_emb_xyz / pos_emb_dir");
    if (!widths && (cfg->pos_emb_xyz < 0 || cfg->pos_emb_xyz > 32 || cfg->pos_emb_dir < 0 || cfg->pos_emb_dir > 32))
        return fail(nullptr, KNERF_ERR_INVALID, "need 0 <= pos_emb_* <= 32");
    // one wavefront walks a ray in compositing (a lane's run of up to 16 samples in registers) and in the sampler (tables in LDS)
    if (!widths && (cfg->n_coarse < 2 || cfg->n_coarse > 512 || cfg->n_fine < 0 || cfg->n_coarse + cfg->n_fine > 1024))
        return fail(nullptr, KNERF_ERR_INVALID, "need 2 <= n_coarse <= 512 and n_coarse + n_fine <= 1024");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, KNERF_ERR_NODEVICE, "no HIP device visible");
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return fail(nullptr, KNERF_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, KNERF_ERR_NODEVICE, std::string("libknerf_hip is built for gfx950 only; device is ") + prop.gcnArchName);
    ctx = new knerf_ctx();
    ctx->cfg = *cfg;
    ctx->opt.lr = cfg->lr;
    // the fused kernels cover the trunk shapes of layout.h KNERF_FUSED_SHAPES (widths 256 and 128; the reference's encodings unless the build added others); everything
    // else -- and, for tests, any shape under KNERF_FLAG_FORCE_GENERIC -- runs on the general-shape kernels
    const int sid = widths ? -1 : fused_shape_id(cfg->n_layers, cfg->skip_layer, cfg->dense_units, cfg->pos_emb_xyz, cfg->pos_emb_dir);
    ctx->generic = sid < 0 || (cfg->flags & KNERF_FLAG_FORCE_GENERIC) != 0;
    ctx->mlp_only = widths;
    if (ctx->generic) {
        ctx->gplan = widths ? gen::build_plan_widths(cfg->n_layers, cfg->dense_units, cfg->skip_layer, cfg->pos_emb_xyz, cfg->pos_emb_dir)
                            : gen::build_plan(cfg->n_layers, cfg->dense_units, cfg->skip_layer, cfg->pos_emb_xyz, cfg->pos_emb_dir);
        ctx->n_params = ctx->gplan.n_params;
    } else {
        ctx->shape = sid; ctx->si = shape_info(sid); ctx->n_params = ctx->si.param_count;
    }
    for (int j = 0; j < ctx->si.n_jobs; ++j) ctx->wgrad_cost[j] = default_wgrad_cost(ctx->si.job_kind[j]);
    const size_t NP = (size_t)ctx->n_params;
    const Tables& ht = host_tables(ctx->shape);
    ctx->tab.host = ht.host; ctx->tab.wgrad = ht.wgrad; ctx->tab.wgrad_off = ht.wgrad_off;
#define CREATECHK(expr)                                                                                          \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                  \
            std::string m_ = std::string(#expr) + ": " + hipGetErrorString(e_);                                  \
            knerf_destroy(ctx);                                                                                  \
            return fail(nullptr, KNERF_ERR_HIP, m_);                                                             \
        }                                                                                                        \
    } while (0)
    CREATECHK(upload(ctx->tab.d_fwd, ctx->tab.host.fwd));
    CREATECHK(upload(ctx->tab.d_bias, ctx->tab.host.fwd_bias));
    CREATECHK(upload(ctx->tab.d_bwd, ctx->tab.host.bwd));
    CREATECHK(upload(ctx->tab.d_wgrad, ctx->tab.wgrad));
    ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (int r = upload_plan(ctx)) { std::string m_ = ctx->err; knerf_destroy(ctx); return fail(nullptr, r, m_); }
    // everything below is allocated zeroed, on the null stream
    CREATECHK(ctx->tile_count.grow(knerf_ctx::kTileCounters, nullptr, true));
    CREATECHK(ctx->tile_stats.grow(8, nullptr, true));       // per net: live, total, [2], [3]: out-of-range list entries (diagnostic builds)
    CREATECHK(ctx->occ_stats.grow(4, nullptr, true));
    CREATECHK(ctx->occ_train_stats.grow(4, nullptr, true));
    CREATECHK(ctx->term_stats.grow(4, nullptr, true));
    CREATECHK(ctx->d_diag.grow(2, nullptr, true));
    CREATECHK(hipHostMalloc(&ctx->h_diag, 4 * sizeof(long long), hipHostMallocDefault));
    ctx->h_diag[0] = ctx->h_diag[1] = ctx->h_diag[2] = ctx->h_diag[3] = 0;
    CREATECHK(ctx->grads.grow(2 * NP, nullptr, true));
    CREATECHK(ctx->aux.grow(2 * (size_t)kAuxCount, nullptr, true));
    CREATECHK(ctx->d_flag.grow(1, nullptr, true));
    CREATECHK(ctx->d_step.grow(1, nullptr, true));
    CREATECHK(ctx->d_lr_t.grow(1, nullptr, true));
    CREATECHK(launch_step_set(0, ctx->d_step, ctx->d_lr_t, AdamHyper{cfg->lr, cfg->beta1, cfg->beta2}, nullptr));
    CREATECHK(hipHostMalloc(&ctx->h_status, 2 * sizeof(int), hipHostMallocDefault));   // written by the device (optim.hip step_status)
    ctx->h_status[0] = ctx->h_status[1] = 0;
    CREATECHK(ctx->loss_tmp.grow(2, nullptr, true));
    CREATECHK(ctx->d_terms.grow(8, nullptr, true));
    for (int n = 0; n < 2; ++n) {
        Net& N = ctx->net[n];
        const size_t NW = ctx->generic ? NP : (size_t)ctx->si.ext_param_count;  // fused path: parameters + composed head (layout.h)
        CREATECHK(N.w.grow(NW, nullptr, true));
        CREATECHK(N.m.grow(NP, nullptr, true));
        CREATECHK(N.v.grow(NP, nullptr, true));
        N.g = ctx->grads + (size_t)n * NP;
        N.aux = ctx->aux + (size_t)n * kAuxCount;
        if (ctx->generic) {
            GenNetBufs& b = ctx->gnet_buf[n];
            CREATECHK(b.packed.grow(ctx->gplan.packed_elems, nullptr, true));
            CREATECHK(b.head.grow(gen::head_floats(ctx->gplan), nullptr, true));
            CREATECHK(b.gaux.grow(gen::aux_floats(ctx->gplan), nullptr, true));
            ctx->gnet[n] = gen::NetDev{b.packed, b.head, b.gaux};
        }
        CREATECHK(N.fwd_stream.grow(stream_bytes(ctx->si.fwd_blocks), nullptr, true));
        CREATECHK(N.bwd_stream.grow(stream_bytes(ctx->si.bwd_blocks), nullptr, true));
        CREATECHK(N.bias.grow((size_t)ctx->si.fwd_bias_tiles * 32, nullptr, true));
    }
    CREATECHK(hipStreamSynchronize(nullptr));       // the zero-fills are done before any stream of the caller's touches the buffers
#undef CREATECHK
    *out = ctx;
    return KNERF_OK;
}

int knerf_destroy(knerf_ctx* ctx) {
    if (!ctx) return KNERF_OK;
    if (ctx->h_status) (void)hipHostFree(ctx->h_status);
    if (ctx->h_diag) (void)hipHostFree(ctx->h_diag);
    for (auto& r : ctx->prof) {             // events of a profile that was never read
        if (r.e0) (void)hipEventDestroy(r.e0);
        if (r.e1) (void)hipEventDestroy(r.e1);
    }
    delete ctx;                             // every device buffer goes with its owner (ctx.h DevBuf)
    return KNERF_OK;
}

int knerf_set_weights(knerf_ctx* ctx, int net, const float* host_flat, size_t n) {
    if (int r = check_net(ctx, net)) return r;
    if (!host_flat || n != (size_t)ctx->n_params) return fail(ctx, KNERF_ERR_INVALID, "weights: expected " + std::to_string(ctx->n_params) + " floats");
    HIPCHK(hipMemcpy(ctx->net[net].w, host_flat, n * sizeof(float), hipMemcpyHostToDevice));
    if (int r = repack(ctx, net, nullptr)) return r;
    HIPCHK(hipStreamSynchronize(nullptr));
    return KNERF_OK;
}

int knerf_get_weights(knerf_ctx* ctx, int net, float* host_flat, size_t n) {
    if (int r = check_net(ctx, net)) return r;
    if (!host_flat || n != (size_t)ctx->n_params) return fail(ctx, KNERF_ERR_INVALID, "weights: expected " + std::to_string(ctx->n_params) + " floats");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host_flat, ctx->net[net].w, n * sizeof(float), hipMemcpyDeviceToHost));
    return KNERF_OK;
}

int knerf_weights_device(knerf_ctx* ctx, int net, float** dev, size_t* n) {
    if (int r = check_net(ctx, net)) return r;
    if (dev) *dev = ctx->net[net].w;
    if (n) *n = (size_t)ctx->n_params;
    return KNERF_OK;
}

int knerf_grads_device(knerf_ctx* ctx, float** dev, size_t* n) {
    if (!ctx) return KNERF_ERR_INVALID;
    if (dev) *dev = ctx->grads;
    if (n) *n = 2 * (size_t)ctx->n_params;
    return KNERF_OK;
}

int knerf_refresh_weights(knerf_ctx* ctx, void* stream) {
    if (!ctx) return KNERF_ERR_INVALID;
    for (int n = 0; n < 2; ++n) if (int r = repack(ctx, n, (hipStream_t)stream)) return r;
    return KNERF_OK;
}

int knerf_forward_chunk(knerf_ctx* ctx, void* stream, int net, const float* o, const float* d, const float* t,
                        int n_rays, int n_samples, float* image, float* depth, float* weights) {
    if (int r = check_net(ctx, net)) return r;
    if (int r = check_rays(ctx, "forward_chunk")) return r;
    if (!o || !d || !t || !image || n_rays <= 0) return fail(ctx, KNERF_ERR_INVALID, "forward_chunk: null/empty argument");
    if (n_samples < 1 || n_samples > ctx->cfg.n_coarse + ctx->cfg.n_fine) return fail(ctx, KNERF_ERR_INVALID, "forward_chunk: n_samples out of range");
    if (int r = ensure_ws(ctx, n_rays, false, (hipStream_t)stream)) return r;
    Pass p{net, o, d, t, n_rays, n_samples};
    p.image = image; p.depth = depth; p.weights = weights;
    return run_pass(ctx, (hipStream_t)stream, p);
}

int knerf_mlp_call(knerf_ctx* ctx, void* stream, int net, const float* xyz_enc, const float* dir_enc, uint64_t n, float* raw) {
    if (int r = check_net(ctx, net)) return r;
    if (!xyz_enc || !dir_enc || !raw || n == 0) return fail(ctx, KNERF_ERR_INVALID, "mlp_call: null/empty argument");
    hipStream_t s = (hipStream_t)stream;
    if (int r = ensure_call(ctx, (long long)n, s)) return r;
    HIPCHK(gen::pack_weights(ctx->call_plan, ctx->net[net].w, ctx->call_net, s));       // the weights may have changed since the last call
    HIPCHK(gen::forward_encoded(ctx->call_plan, ctx->call_ws, ctx->call_net, ctx->net[net].w, xyz_enc, dir_enc, (long long)n, raw, s));
    return KNERF_OK;
}

int knerf_query_points(knerf_ctx* ctx, void* stream, int net, const float* xyz, const float* dirs, int dir_per_point, uint64_t n,
                       float* raw, float* sigma, float* rgb) {
    if (int r = check_net(ctx, net)) return r;
    if (int r = check_rays(ctx, "query_points")) return r;
    if (!xyz) return fail(ctx, KNERF_ERR_INVALID, "query_points: null xyz");
    QueryArgs q{};
    q.xyz = xyz; q.dir = dirs; q.dir_stride = dir_per_point ? 3 : 0; q.grid = 0;
    q.raw = raw; q.sigma = sigma; q.rgb = rgb; q.n = (long long)n;
    return run_query(ctx, stream, net, q);
}

int knerf_query_grid(knerf_ctx* ctx, void* stream, int net, const int32_t* resolution, const float* lo, const float* hi, const float* dir,
                     float* raw, float* sigma, float* rgb) {
    if (int r = check_net(ctx, net)) return r;
    if (int r = check_rays(ctx, "query_grid")) return r;
    if (!resolution || !lo || !hi) return fail(ctx, KNERF_ERR_INVALID, "query_grid: null resolution / lo / hi");
    QueryArgs q{};
    q.grid = 1; q.dir = dir; q.dir_stride = 0;
    long long n = 1;
    for (int a = 0; a < 3; ++a) {
        if (resolution[a] < 2) return fail(ctx, KNERF_ERR_INVALID, "query_grid: every resolution must be >= 2");
        if (!(hi[a] > lo[a])) return fail(ctx, KNERF_ERR_INVALID, "query_grid: need hi > lo on every axis");
        q.gr[a] = resolution[a];
        q.lo[a] = lo[a];
        q.step[a] = (hi[a] - lo[a]) / (float)(resolution[a] - 1);      // fp32 subtraction and division, as NumPy's float32
        n *= resolution[a];
    }
    q.raw = raw; q.sigma = sigma; q.rgb = rgb; q.n = n;
    return run_query(ctx, stream, net, q);
}

int knerf_set_occupancy(knerf_ctx* ctx, void* stream, int net, const uint32_t* bits, const int32_t* cells, const float* lo, const float* hi,
                        int outside_empty) {
    if (int r = check_net(ctx, net)) return r;
    if (int r = check_rays(ctx, "set_occupancy")) return r;
    hipStream_t s = (hipStream_t)stream;
    knerf_ctx::Occ& G = ctx->occ[net];
    if (!bits) {                                        // detach: passes enqueued earlier may still read the old bits
        HIPCHK(hipStreamSynchronize(s));
        G.bits.reset();
        G.grid = OccGrid{};
        return KNERF_OK;
    }
    if (!cells || !lo || !hi) return fail(ctx, KNERF_ERR_INVALID, "set_occupancy: null cells / lo / hi");
    float scale[3];
    long long n = 1;
    for (int a = 0; a < 3; ++a) {
        if (cells[a] < 1 || cells[a] > 1024) return fail(ctx, KNERF_ERR_INVALID, "set_occupancy: need 1 <= cells <= 1024 on every axis");
        if (!(hi[a] > lo[a]) || !std::isfinite(lo[a]) || !std::isfinite(hi[a])) return fail(ctx, KNERF_ERR_INVALID, "set_occupancy: need finite hi > lo on every axis");
        scale[a] = (float)((double)cells[a] / ((double)hi[a] - (double)lo[a]));
        if (!std::isfinite(scale[a])) return fail(ctx, KNERF_ERR_INVALID, "set_occupancy: the box is too thin for its cells");
        n *= cells[a];
    }
    const size_t words = (size_t)((n + 31) / 32);
    G.grid.bits = nullptr;
    HIPCHK(G.bits.grow(words, s));
    HIPCHK(hipMemcpyAsync(G.bits, bits, words * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));     // behind every pass enqueued earlier
    G.grid.bits = G.bits;
    for (int a = 0; a < 3; ++a) { G.grid.cells[a] = cells[a]; G.grid.lo[a] = lo[a]; G.grid.scale[a] = scale[a]; }
    G.grid.outside_empty = outside_empty ? 1 : 0;
    return KNERF_OK;
}

// [net][k] counters whose first two per net are (live, total): read behind the stream, optionally reset; all: null, or all 2 k <= 8 words
static int read_stats(knerf_ctx* ctx, void* stream, DevBuf<long long> knerf_ctx::*which, int64_t* live, int64_t* total, int reset, long long* all = nullptr) {
    if (!ctx || !live || !total) return KNERF_ERR_INVALID;
    long long own[8];
    long long* h = all ? all : own;
    const DevBuf<long long>& words = ctx->*which;
    const int k = (int)words.size() / 2;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipMemcpy(h, words, words.bytes(), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(words, 0, words.bytes()));
    for (int n = 0; n < 2; ++n) { live[n] = h[k * n]; total[n] = h[k * n + 1]; }
    return KNERF_OK;
}

int knerf_occupancy_stats(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset) {
    return read_stats(ctx, stream, &knerf_ctx::occ_stats, live, total, reset);
}

int knerf_occupancy_train_stats(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset) {
    return read_stats(ctx, stream, &knerf_ctx::occ_train_stats, live, total, reset);
}

int knerf_termination_stats(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset) {
    return read_stats(ctx, stream, &knerf_ctx::term_stats, live, total, reset);
}

int knerf_sample_fine(knerf_ctx* ctx, void* stream, const float* t_coarse, const float* w_coarse, const float* u,
                      uint64_t seed, uint64_t stream_id, uint64_t ray_offset, int n_rays, float* t_out) {
    if (int r = check_rays(ctx, "sample_fine")) return r;
    if (!t_coarse || !w_coarse || !t_out || n_rays <= 0) return fail(ctx, KNERF_ERR_INVALID, "sample_fine: null/empty argument");
    SampleArgs sa{};
    sa.t_coarse = t_coarse; sa.w_coarse = w_coarse; sa.u = u; sa.t_out = t_out; sa.R = n_rays;
    sa.Nc = ctx->cfg.n_coarse; sa.Nf = ctx->cfg.n_fine; sa.oob_clamp = ctx->cfg.oob_clamp;
    sa.seed = seed; sa.stream_id = stream_id; sa.ray_offset = ray_offset;
    { ProfScope ps(ctx, (hipStream_t)stream, P_SAMPLE); HIPCHK(launch_sample_fine(sa, (hipStream_t)stream)); }
    return KNERF_OK;
}

int knerf_render_chunk(knerf_ctx* ctx, void* stream, const float* o, const float* d, const float* t, const float* u,
                       uint64_t seed, uint64_t ray_offset, int n_rays, float* c_image, float* c_depth, float* c_weights,
                       float* f_image, float* f_depth, float* f_weights, float* t_fine) {
    if (int r = check_rays(ctx, "render_chunk")) return r;
    if (!o || !d || !t || !c_image || !f_image || n_rays <= 0) return fail(ctx, KNERF_ERR_INVALID, "render_chunk: null/empty argument");
    hipStream_t s = (hipStream_t)stream;
    if (int r = ensure_ws(ctx, n_rays, false, s)) return r;
    const int Nc = ctx->cfg.n_coarse, Na = Nc + ctx->cfg.n_fine;
    float* wc = c_weights ? c_weights : ctx->w_c.get();
    float* tf = t_fine ? t_fine : ctx->t_f.get();
    Pass p{KNERF_COARSE, o, d, t, n_rays, Nc};
    p.image = c_image; p.depth = c_depth; p.weights = wc; p.render = true;
    if (int r = run_pass(ctx, s, p)) return r;
    if (int r = knerf_sample_fine(ctx, stream, t, wc, u, seed, 0, ray_offset, n_rays, tf)) return r;
    p.net = KNERF_FINE; p.t = tf; p.S = Na;
    p.image = f_image; p.depth = f_depth; p.weights = f_weights;
    return run_pass(ctx, s, p);
}

int knerf_render_batch(knerf_ctx* ctx, void* stream, const float* o, const float* d, const float* t, const float* u, uint64_t seed,
                       int n_rays, int ray_chunks, float* c_image, float* c_depth, float* c_weights, float* f_image, float* f_depth,
                       float* f_weights, float* t_fine) {
    if (int r = check_rays(ctx, "render_batch")) return r;            // (before any workspace is sized: a stand-alone-MLP context has none)
    if (ray_chunks <= 0 || n_rays <= 0 || n_rays % ray_chunks != 0)
        return fail(ctx, KNERF_ERR_INVALID, "render_batch: ray_chunks must be a divisor of the number of rays");   // nerf.py:100
    const size_t Nc = (size_t)ctx->cfg.n_coarse, Nf = (size_t)ctx->cfg.n_fine, Na = Nc + Nf;
    // per-ray work only: bit-identical outputs.  Rendering keeps no saved tensors (5 KB of workspace per ray on the fused path), so its
    // launches may be far larger than a training step's: 65,536 rays by default ("merge_render_rays"; a 256 x 256 frame in ONE set
    // of launches is 4 % faster than in sixteen); the general-shape path's activations stay in memory, it keeps the training limit
    // ... and `ray_chunks` stays the reference's memory knob: merged launches that do not fit fall back to the caller's own chunks
    // (remembered per (ray_chunks, chunk count), so that later frames do not fail the same allocation again)
    const int user_chunks = ray_chunks, user_n = n_rays / ray_chunks;
    int m = merge_factor(ctx->generic ? ctx->merge_rays : ctx->merge_render_rays, ray_chunks, user_n);
    if (m > 1 && ctx->rmerge_fail_rays == user_chunks && ctx->rmerge_fail_chunks == user_n) m = 1;
    if (m > 1 && ensure_ws(ctx, user_chunks * m, false, (hipStream_t)stream)) {
        ctx->rmerge_fail_rays = user_chunks; ctx->rmerge_fail_chunks = user_n; ++ctx->merge_fallbacks;
        m = 1;
    }
    ray_chunks = user_chunks * m;
    for (int i = 0; i < n_rays / ray_chunks; ++i) {
        const size_t r0 = (size_t)i * ray_chunks;
        if (int r = knerf_render_chunk(ctx, stream, o + r0 * 3, d + r0 * 3, t + r0 * Nc, u ? u + r0 * Nf : nullptr, seed, (uint64_t)r0,
                                       ray_chunks, c_image ? c_image + r0 * 3 : nullptr, c_depth ? c_depth + r0 : nullptr,
                                       c_weights ? c_weights + r0 * Nc : nullptr, f_image ? f_image + r0 * 3 : nullptr,
                                       f_depth ? f_depth + r0 : nullptr, f_weights ? f_weights + r0 * Na : nullptr,
                                       t_fine ? t_fine + r0 * Na : nullptr))
            return r;
    }
    return KNERF_OK;
}

int knerf_train_chunk(knerf_ctx* ctx, void* stream, const float* o, const float* d, const float* t, const float* target,
                      const float* u, uint64_t seed, uint64_t ray_offset, int n_rays, float inv_chunks, float* loss,
                      float* c_image, float* f_image) {
    if (int r = check_rays(ctx, "train_chunk")) return r;
    if (!o || !d || !t || !target || n_rays <= 0) return fail(ctx, KNERF_ERR_INVALID, "train_chunk: null/empty argument");
    hipStream_t s = (hipStream_t)stream;
    if (ctx->plan_dirty) { if (int r = upload_plan(ctx)) return r; }
    ctx->tile_counter_next = 0;
    if (int r = ensure_ws(ctx, n_rays, true, s)) return r;
    if (int r = train_chunk_impl(ctx, s, Chunk{o, d, t, target, u, seed, ray_offset, n_rays, inv_chunks, loss, c_image, f_image})) return r;
    return expand_head_grads(ctx, s);
}

int knerf_train_batch(knerf_ctx* ctx, void* stream, const float* o, const float* d, const float* t, const float* target,
                      const float* u, uint64_t seed, int n_rays, int ray_chunks, float* loss, float* c_image, float* f_image) {
    if (int r = check_rays(ctx, "train_batch")) return r;
    if (!o || !d || !t || !target) return fail(ctx, KNERF_ERR_INVALID, "train_batch: null argument");
    if (ray_chunks <= 0 || n_rays <= 0 || n_rays % ray_chunks != 0)
        return fail(ctx, KNERF_ERR_INVALID, "train_batch: ray_chunks must be a divisor of the number of rays");   // nerf.py:100
    hipStream_t s = (hipStream_t)stream;
    const int Nc = ctx->cfg.n_coarse, Nf = ctx->cfg.n_fine;
    if (ctx->plan_dirty) { if (int r = upload_plan(ctx)) return r; }
    ctx->tile_counter_next = 0;
    if (ctx->obj_ext) HIPCHK(hipMemsetAsync(ctx->d_terms, 0, 8 * sizeof(float), s));      // knerf_objective_terms: of this batch
    // zero-gradient diagnostics count the LAST chunk's gradient (nerf.py:430-451): that chunk's launches must be its own
    int merge = ctx->grad_diag ? 1 : merge_factor(ctx->merge_rays, ray_chunks, n_rays / ray_chunks);
    const int user_chunks = ray_chunks;
    if (merge > 1 && ctx->merge_fail_rays == user_chunks && ctx->merge_fail_chunks == n_rays / user_chunks) merge = 1;   // did not fit last time
    int C = 0, G = 1;
    for (;;) {
        ray_chunks = user_chunks * merge;
        C = n_rays / ray_chunks;
        G = ctx->grad_diag ? 1 : wgrad_group_for(ctx, ray_chunks, C);
        int r = ensure_ws(ctx, ray_chunks, true, s, G);
        if (r && G > 1) {                                           // the group did not fit: one chunk per wgrad launch
            G = 1;
            ctx->group_cache_rays = ray_chunks; ctx->group_cache_chunks = C; ctx->group_cache = 1;
            r = ensure_ws(ctx, ray_chunks, true, s, 1);
        }
        if (!r) break;
        if (merge == 1) return r;
        merge = 1;                                                  // the merged launches did not fit either: the caller's own chunks
        ctx->merge_fail_rays = user_chunks; ctx->merge_fail_chunks = n_rays / user_chunks; ++ctx->merge_fallbacks;
    }
    const size_t tc = ws_sizes(ctx, ray_chunks).tiles_c;
    const bool skip = skipping(ctx);
    // coarse passes on the compacted path (occupancy_train): their flags lie at tile_flags + slot tc, a group's list is compacted from them
    const bool occ_c = !ctx->generic && occ_train_on(ctx, KNERF_COARSE);
    if (skip || (!ctx->generic && occ_train_any(ctx))) { if (int r = ensure_tile_counters(ctx, s, 2LL * C + (C + G - 1) / G + 8)) return r; }   // two passes per chunk + one per group
    const bool append_g = G > 1 && skip && !ctx->deterministic && !occ_c;
    int* group_count = nullptr;
    for (int i = 0; i < C; ++i) {
        const size_t r0 = (size_t)i * ray_chunks;
        const int slot = i % G;
        const bool last = slot == G - 1 || i == C - 1;
        if (ctx->grad_diag && i == C - 1 && C > 1) {
            // set the sum of the earlier chunks aside (head sums expanded first: the expansion is linear), so that the accumulator
            // holds the last chunk's gradient alone when it is counted
            if (int r = expand_head_grads(ctx, s)) return r;
            HIPCHK(ctx->diag_tmp.grow(ctx->grads.size(), s));
            HIPCHK(hipMemcpyAsync(ctx->diag_tmp, ctx->grads, ctx->grads.bytes(), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemsetAsync(ctx->grads, 0, ctx->grads.bytes(), s));
        }
        // default-mode skipping: the coarse passes of a group append their live tiles to the group's list under one counter
        if (append_g && slot == 0) { if (int r = next_tile_counter(ctx, s, &group_count)) return r; }
        Chunk c{o + r0 * 3, d + r0 * 3, t + r0 * Nc, target + r0 * 3, u ? u + r0 * Nf : nullptr, seed, (uint64_t)r0, ray_chunks, 1.0f / (float)C,
                loss, c_image ? c_image + r0 * 3 : nullptr, f_image ? f_image + r0 * 3 : nullptr};
        c.slot = slot; c.group = G; c.group_count = append_g ? group_count : nullptr;
        if (int r = train_chunk_impl(ctx, s, c)) return r;
        if (G > 1 && last) {                                        // the group's coarse weight gradients in one launch
            const int* live = nullptr; int* live_count = nullptr;
            if (occ_c) {                                            // compacted coarse passes: every flag of each region counts (zero past its list)
                if (int r = compact_tiles(ctx, s, ctx->tile_flags, (int)((slot + 1) * tc), (int)tc, (int)tc, ctx->tile_list, &live_count)) return r;
                live = ctx->tile_list;
            } else if (skip && ctx->deterministic) {                // ascending list of the group's live tiles from its flags
                if (int r = compact_tiles(ctx, s, ctx->tile_flags, (int)((slot + 1) * tc), (int)tc, ray_chunks * Nc / kTile, ctx->tile_list, &live_count)) return r;
                live = ctx->tile_list;
            } else if (skip) {
                live = ctx->tile_list_g; live_count = group_count;
            }
            if (int r = launch_wgrad_tiles(ctx, s, KNERF_COARSE, 0, (size_t)(slot + 1) * tc, live, live_count)) return r;
        }
    }
    if (int r = expand_head_grads(ctx, s)) return r;
    if (ctx->grad_diag) {
        HIPCHK(launch_grad_diagnostics(ctx->grads, ctx->n_params, ctx->d_diag, ctx->h_diag, s));
        if (C > 1) HIPCHK(launch_add_into(ctx->grads, ctx->diag_tmp, 2 * (size_t)ctx->n_params, s));
    }
    return KNERF_OK;
}

// ---- optimizer options (include/knerf.h knerf_set_optimizer; optim_ext.h) ------------------------------------------------------
static SchedArgs sched_args(const knerf_ctx* ctx) {
    const knerf_optimizer& o = ctx->opt;
    SchedArgs a{};
    a.kind = o.schedule; a.staircase = o.staircase; a.n_values = o.n_values;
    a.lr = o.lr; a.decay_steps = o.decay_steps; a.decay_rate = o.decay_rate; a.alpha = o.alpha; a.weight_decay = o.weight_decay;
    for (int i = 0; i < KNERF_SCHEDULE_MAX_VALUES - 1; ++i) a.boundaries[i] = o.boundaries[i];
    for (int i = 0; i < KNERF_SCHEDULE_MAX_VALUES; ++i) a.values[i] = o.values[i];
    a.b1 = ctx->cfg.beta1; a.b2 = ctx->cfg.beta2;
    return a;
}
// device tables and buffers of the extended step, once per context: the tensors of one net in Keras order (mlp.py:11-27: layer_i
// kernel [in, units] and bias, then sigma, features, rgb_features, rgb) and their cut into items of the sum-of-squares pass
static int ensure_opt_buffers(knerf_ctx* ctx) {
    if (ctx->d_opt_tab) return KNERF_OK;
    const knerf_config& c = ctx->cfg;
    const bool widths = (c.flags & KNERF_FLAG_ENCODED_WIDTHS) != 0;
    const int xyz = widths ? c.pos_emb_xyz : 3 + 6 * c.pos_emb_xyz, dir = widths ? c.pos_emb_dir : 3 + 6 * c.pos_emb_dir, U = c.dense_units;
    std::vector<int32_t> off{0};
    auto dense = [&](int fan_in, int fan_out) { off.push_back(off.back() + fan_in * fan_out); off.push_back(off.back() + fan_out); };
    int fan_in = xyz;
    for (int i = 0; i < c.n_layers; ++i) {
        dense(fan_in, U);
        fan_in = (i % c.skip_layer == 0 && i > 0) ? U + xyz : U;
    }
    dense(fan_in, 1); dense(fan_in, U); dense(U + dir, U / 2); dense(U / 2, 3);
    const int T = (int)off.size() - 1;
    if (off.back() != ctx->n_params || T > kOptMaxTensors) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: the tensor list does not match the parameter count");
    std::vector<int32_t> item0{0}, begin, end;
    for (int t = 0; t < T; ++t) {
        for (int b = off[t]; b < off[t + 1]; b += kOptItemElems) { begin.push_back(b); end.push_back(std::min(b + kOptItemElems, off[t + 1])); }
        item0.push_back((int32_t)begin.size());
    }
    const int I = (int)begin.size();
    std::vector<int32_t> tab(off);
    tab.insert(tab.end(), item0.begin(), item0.end()); tab.insert(tab.end(), begin.begin(), begin.end()); tab.insert(tab.end(), end.begin(), end.end());
    HIPCHK(ctx->d_opt_partial.grow(2 * (size_t)I, nullptr, true));
    HIPCHK(ctx->d_opt_f.grow(1 + 2 * (size_t)kOptMaxTensors, nullptr, true));
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(upload(ctx->d_opt_tab, tab));           // last: its presence says that all three are there
    ctx->opt_tensors = T; ctx->opt_items = I;
    return KNERF_OK;
}

int knerf_set_optimizer(knerf_ctx* ctx, void* stream, const knerf_optimizer* opt) {
    if (!ctx) return KNERF_ERR_INVALID;
    if (!opt) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: null argument");
    if (ctx->mlp_only) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: a KNERF_FLAG_ENCODED_WIDTHS context has no optimizer");
    knerf_optimizer o = *opt;
    auto ok = [](double v) { return std::isfinite(v) && v >= 0; };
    if (o.schedule < KNERF_SCHEDULE_CONSTANT || o.schedule > KNERF_SCHEDULE_PIECEWISE) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: unknown schedule kind " + std::to_string(o.schedule));
    if (o.clip != KNERF_CLIP_NONE && o.clip != KNERF_CLIP_VALUE && o.clip != KNERF_CLIP_NORM && o.clip != KNERF_CLIP_GLOBAL_NORM)
        return fail(ctx, KNERF_ERR_INVALID, (o.clip > 0 && o.clip < 8) ? "set_optimizer: at most one of clipvalue, clipnorm and global_clipnorm may be active"
                                                                      : "set_optimizer: unknown clip kind " + std::to_string(o.clip));
    if (o.clip != KNERF_CLIP_NONE && !(ok(o.clip_arg) && o.clip_arg > 0)) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: the clip argument must be finite and > 0");
    if (!ok(o.weight_decay)) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: weight_decay must be finite and >= 0");
    if (o.schedule != KNERF_SCHEDULE_PIECEWISE && !ok(o.lr)) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: the learning rate must be finite and >= 0");
    if (o.schedule == KNERF_SCHEDULE_EXPONENTIAL || o.schedule == KNERF_SCHEDULE_COSINE) {
        if (!(std::isfinite(o.decay_steps) && o.decay_steps > 0)) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: decay_steps must be finite and > 0");
        if (o.schedule == KNERF_SCHEDULE_EXPONENTIAL && !ok(o.decay_rate)) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: decay_rate must be finite and >= 0");
        if (o.schedule == KNERF_SCHEDULE_COSINE && !ok(o.alpha)) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: alpha must be finite and >= 0");
    }
    if (o.schedule == KNERF_SCHEDULE_PIECEWISE) {
        if (o.n_values < 1 || o.n_values > KNERF_SCHEDULE_MAX_VALUES)
            return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: a piecewise schedule takes 1.." + std::to_string(KNERF_SCHEDULE_MAX_VALUES) + " values, got " + std::to_string(o.n_values));
        for (int i = 0; i < o.n_values; ++i)
            if (!ok(o.values[i])) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: piecewise values must be finite and >= 0");
        for (int i = 0; i + 1 < o.n_values; ++i)
            if (o.boundaries[i] < 0 || (i > 0 && o.boundaries[i] <= o.boundaries[i - 1])) return fail(ctx, KNERF_ERR_INVALID, "set_optimizer: piecewise boundaries must be >= 0 and ascend");
    }
    // what the chosen kinds do not read is stored as zero, so that knerf_get_optimizer returns a canonical record
    if (o.schedule != KNERF_SCHEDULE_EXPONENTIAL) { o.staircase = 0; o.decay_rate = 0; }
    if (o.schedule != KNERF_SCHEDULE_EXPONENTIAL && o.schedule != KNERF_SCHEDULE_COSINE) o.decay_steps = 0;
    if (o.schedule != KNERF_SCHEDULE_COSINE) o.alpha = 0;
    if (o.schedule != KNERF_SCHEDULE_PIECEWISE) o.n_values = 0; else o.lr = 0;
    for (int i = 0; i < KNERF_SCHEDULE_MAX_VALUES; ++i) if (i >= o.n_values) o.values[i] = 0;
    for (int i = 0; i < KNERF_SCHEDULE_MAX_VALUES - 1; ++i) if (i + 1 >= o.n_values) o.boundaries[i] = 0;
    o.staircase = o.staircase != 0;
    if (o.clip == KNERF_CLIP_NONE) o.clip_arg = 0;
    if (o.schedule == KNERF_SCHEDULE_CONSTANT) o.lr = (double)(float)o.lr;          // held as fp32, as knerf_config.lr: the plain kernels' rate
    const bool ext = o.schedule != KNERF_SCHEDULE_CONSTANT || o.clip != KNERF_CLIP_NONE || o.weight_decay > 0;
    if (ext)
        if (int r = ensure_opt_buffers(ctx)) return r;
    ctx->opt = o; ctx->opt_ext = ext;
    hipStream_t s = (hipStream_t)stream;
    if (ext) {
        HIPCHK(launch_step_set_ext(-1, ctx->d_step, ctx->d_lr_t, o.weight_decay > 0 ? ctx->d_opt_f : nullptr, sched_args(ctx), s));
    } else {
        ctx->cfg.lr = (float)o.lr;
        HIPCHK(launch_step_set_ext(-1, ctx->d_step, ctx->d_lr_t, nullptr, sched_args(ctx), s));      // (a constant schedule: keras_lr_t's bits)
    }
    return KNERF_OK;
}

int knerf_get_optimizer(knerf_ctx* ctx, knerf_optimizer* opt) {
    if (!ctx || !opt) return KNERF_ERR_INVALID;
    *opt = ctx->opt;
    return KNERF_OK;
}

// ---- the objective (include/knerf.h knerf_set_objective; composite_ext.h) -------------------------------------------------------
int knerf_set_objective(knerf_ctx* ctx, void* stream, const knerf_objective* obj) {
    if (!ctx) return KNERF_ERR_INVALID;
    if (!obj) return fail(ctx, KNERF_ERR_INVALID, "set_objective: null argument");
    if (ctx->mlp_only) return fail(ctx, KNERF_ERR_INVALID, "set_objective: a KNERF_FLAG_ENCODED_WIDTHS context has no train step");
    knerf_objective o = *obj;
    auto ok = [](float v) { return std::isfinite(v) && v >= 0; };
    if (o.loss_kind < KNERF_LOSS_MSE || o.loss_kind > KNERF_LOSS_LOG_COSH) return fail(ctx, KNERF_ERR_INVALID, "set_objective: unknown loss kind " + std::to_string(o.loss_kind));
    if (o.loss_kind == KNERF_LOSS_HUBER && !(std::isfinite(o.huber_delta) && o.huber_delta > 0)) return fail(ctx, KNERF_ERR_INVALID, "set_objective: huber_delta must be finite and > 0");
    if (!ok(o.distortion)) return fail(ctx, KNERF_ERR_INVALID, "set_objective: the distortion weight must be finite and >= 0");
    if (!ok(o.opacity_entropy)) return fail(ctx, KNERF_ERR_INVALID, "set_objective: the opacity_entropy weight must be finite and >= 0");
    if (o.nets < 1 || o.nets > 3) return fail(ctx, KNERF_ERR_INVALID, "set_objective: nets must be 1 (coarse), 2 (fine) or 3 (both), got " + std::to_string(o.nets));
    // what the chosen kind does not read is stored as zero, so that knerf_get_objective returns a canonical record
    if (o.loss_kind != KNERF_LOSS_HUBER) o.huber_delta = 0;
    if (o.distortion == 0 && o.opacity_entropy == 0) { o.distortion = 0; o.opacity_entropy = 0; o.nets = 3; }
    ctx->obj = o;
    ctx->obj_ext = o.loss_kind != KNERF_LOSS_MSE || o.distortion > 0 || o.opacity_entropy > 0;
    HIPCHK(hipMemsetAsync(ctx->d_terms, 0, 8 * sizeof(float), (hipStream_t)stream));
    return KNERF_OK;
}

int knerf_get_objective(knerf_ctx* ctx, knerf_objective* obj) {
    if (!ctx || !obj) return KNERF_ERR_INVALID;
    *obj = ctx->obj;
    return KNERF_OK;
}

int knerf_objective_terms(knerf_ctx* ctx, void* stream, float* out) {
    if (!ctx) return KNERF_ERR_INVALID;
    if (!out) return fail(ctx, KNERF_ERR_INVALID, "objective_terms: null argument");
    if (ctx->mlp_only) return fail(ctx, KNERF_ERR_INVALID, "objective_terms: a KNERF_FLAG_ENCODED_WIDTHS context has no train step");
    HIPCHK(hipMemcpyAsync(out, ctx->d_terms, 8 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return KNERF_OK;
}

int knerf_get_adam_state(knerf_ctx* ctx, void* stream, int net, float* m_host, float* v_host, size_t n) {
    if (int r = check_net(ctx, net)) return r;
    if (!m_host || !v_host || n != (size_t)ctx->n_params) return fail(ctx, KNERF_ERR_INVALID, "adam state: expected two arrays of " + std::to_string(ctx->n_params) + " floats");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipMemcpy(m_host, ctx->net[net].m, n * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(v_host, ctx->net[net].v, n * sizeof(float), hipMemcpyDeviceToHost));
    return KNERF_OK;
}

int knerf_set_adam_state(knerf_ctx* ctx, void* stream, int net, const float* m_host, const float* v_host, size_t n) {
    if (int r = check_net(ctx, net)) return r;
    if (!m_host || !v_host || n != (size_t)ctx->n_params) return fail(ctx, KNERF_ERR_INVALID, "adam state: expected two arrays of " + std::to_string(ctx->n_params) + " floats");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipMemcpy(ctx->net[net].m, m_host, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->net[net].v, v_host, n * sizeof(float), hipMemcpyHostToDevice));
    return KNERF_OK;
}

// Finite check first, on the device; the Adam kernels read its flag and leave weights and slots untouched when it is set (the
// reference aborts fit at nerf.py:381-382).  Nothing here waits for the GPU: the outcome reaches the host through a pinned status
// word (knerf_poll_nonfinite).
// While an optimizer extension is active (knerf_set_optimizer; optim_ext.h): the same sequence with the extended element-wise and step
// kernels; the norm kinds of clipping replace the finite check by the sum-of-squares pass that contains it and add one launch (the
// ordered pass that turns the partial sums into factors).
int knerf_apply_adam(knerf_ctx* ctx, void* stream) {
    if (!ctx) return KNERF_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const knerf_optimizer& o = ctx->opt;
    const bool ext = ctx->opt_ext;
    const int T = ctx->opt_tensors, I = ctx->opt_items;
    const int* tensor_off = ctx->d_opt_tab;
    float* decay = ext && o.weight_decay > 0 ? ctx->d_opt_f.get() : nullptr;
    HIPCHK(hipMemsetAsync(ctx->d_flag, 0, sizeof(int), s));
    if (ext && (o.clip == KNERF_CLIP_NORM || o.clip == KNERF_CLIP_GLOBAL_NORM)) {
        const int *tensor_item0 = tensor_off + T + 1, *item_begin = tensor_item0 + T + 1, *item_end = item_begin + I;
        HIPCHK(launch_sumsq_partial(ctx->grads, ctx->n_params, item_begin, item_end, I, ctx->d_opt_partial, ctx->d_flag, s));
        HIPCHK(launch_clip_scale(ctx->d_opt_partial, I, tensor_item0, T, o.clip, o.clip_arg, ctx->d_opt_f + 1, s));
    } else {
        HIPCHK(launch_check_finite(ctx->grads, 2 * ctx->n_params, ctx->d_flag, s));
    }
    ctx->step += 1;           // host mirror: steps enqueued minus the skipped ones that have been polled; Adam's t lives on the device
    ProfScope ps(ctx, s, P_ADAM);
    for (int n = 0; n < 2; ++n) {
        AdamExtArgs x{};
        AdamArgs& a = x.a;
        a.w = ctx->net[n].w; a.m = ctx->net[n].m; a.v = ctx->net[n].v; a.g = ctx->net[n].g; a.n = ctx->n_params;
        a.lr_t = ctx->d_lr_t; a.b1 = ctx->cfg.beta1; a.b2 = ctx->cfg.beta2; a.eps = ctx->cfg.epsilon; a.nonfinite = ctx->d_flag;
        if (ext) {
            x.clip = o.clip; x.clip_value = (float)o.clip_arg; x.scale = ctx->d_opt_f + 1 + n * kOptMaxTensors; x.tensor_off = tensor_off; x.n_tensors = T;
            x.decay = decay;
            HIPCHK(launch_adam_ext(x, s));
        } else {
            HIPCHK(launch_adam(a, s));
        }
    }
    if (!ctx->generic) HIPCHK(launch_head_compose(ctx->net[0].w, ctx->net[1].w, ctx->si.trunk_params, ctx->si.units, ctx->si.trunk_x, ctx->si.trunk_x_slots, ctx->si.dir_dim, ctx->si.dir_slots, s));      // both nets' heads in one launch
    for (int n = 0; n < 2; ++n)
        if (int r = repack(ctx, n, s, false)) return r;
    if (ext) HIPCHK(launch_step_status_ext(ctx->d_flag, ctx->h_status, ctx->d_step, ctx->d_lr_t, decay, sched_args(ctx), s));
    else HIPCHK(launch_step_status(ctx->d_flag, ctx->h_status, ctx->d_step, ctx->d_lr_t, AdamHyper{ctx->cfg.lr, ctx->cfg.beta1, ctx->cfg.beta2}, s));
    return KNERF_OK;
}

int knerf_poll_nonfinite(knerf_ctx* ctx, void* stream, int wait) {
    if (!ctx) return KNERF_ERR_INVALID;
    if (wait) HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    const int skipped = *reinterpret_cast<volatile int*>(ctx->h_status);
    if (skipped != ctx->skipped_seen) {
        ctx->step -= skipped - ctx->skipped_seen;          // those updates did not happen: the step counter (Adam's t) goes back
        ctx->skipped_seen = skipped;
        return fail(ctx, KNERF_ERR_NONFINITE, "Gradient is not finite");
    }
    return KNERF_OK;
}

int knerf_zero_grads(knerf_ctx* ctx, void* stream) {
    if (!ctx) return KNERF_ERR_INVALID;
    HIPCHK(hipMemsetAsync(ctx->grads, 0, 2 * (size_t)ctx->n_params * sizeof(float), (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(ctx->aux, 0, 2 * (size_t)kAuxCount * sizeof(float), (hipStream_t)stream));
    if (ctx->generic)
        for (int n = 0; n < 2; ++n) HIPCHK(hipMemsetAsync(ctx->gnet[n].gaux, 0, gen::aux_floats(ctx->gplan) * sizeof(float), (hipStream_t)stream));
    return KNERF_OK;
}

int knerf_set_option(knerf_ctx* ctx, const char* name, double value) {
    if (!ctx || !name) return KNERF_ERR_INVALID;
    const std::string n(name);
    if (n == "deterministic") {
        ctx->deterministic = value != 0;         // fused path: wgrad slabs + wgrad_reduce_kernel; general-shape path: generic.hip's slabs (round 5)
    } else if (n == "grad_diagnostics") {
        ctx->grad_diag = value != 0;
    } else if (n == "skip_dead_tiles") {
        ctx->skip_dead = value != 0;               // ignored where it does not apply (general-shape path, sample counts not multiples of 32)
    } else if (n == "occupancy_train") {
        if (value != 0 && value != 1) return fail(ctx, KNERF_ERR_INVALID, "occupancy_train: 0 or 1");
        ctx->occ_train = value != 0;               // applies to the nets with a grid attached (knerf_set_occupancy)
    } else if (n == "termination_threshold") {
        if (!std::isfinite(value) || value < 0 || value >= 1) return fail(ctx, KNERF_ERR_INVALID, "termination_threshold: a finite eps in [0, 1)");
        ctx->term_eps = value;                     // 0: off (render passes as without the option, bit for bit)
    } else if (n == "termination_segment") {
        if (!(value >= 1 && value <= 1024) || value != std::floor(value)) return fail(ctx, KNERF_ERR_INVALID, "termination_segment: an integer 1..1024");
        ctx->term_L = (int)value;
    } else if (n == "merge_chunk_rays") {
        if (value < 0 || value > 1048576) return fail(ctx, KNERF_ERR_INVALID, "merge_chunk_rays: 0..1048576");
        ctx->merge_rays = (int)value; ctx->merge_fail_rays = 0; if (ctx->generic) ctx->rmerge_fail_rays = 0;
    } else if (n == "merge_render_rays") {
        if (value < 0 || value > 1048576) return fail(ctx, KNERF_ERR_INVALID, "merge_render_rays: 0..1048576");
        ctx->merge_render_rays = (int)value; ctx->rmerge_fail_rays = 0;
    } else if (n == "workspace_limit_gb") {      // tests: workspace requests above it fail like an exhausted device (0 = off)
        if (value < 0) return fail(ctx, KNERF_ERR_INVALID, "workspace_limit_gb: >= 0");
        ctx->ws_limit_gb = value; ctx->merge_fail_rays = ctx->rmerge_fail_rays = 0; ctx->group_cache = 0;
    } else if (n == "wgrad_group_max") {
        if (value < 1 || value > 64) return fail(ctx, KNERF_ERR_INVALID, "wgrad_group_max: 1..64");
        ctx->wgrad_group_max = (int)value; ctx->group_cache = 0;
    } else if (n == "wgrad_group_gb") {
        if (value < 0) return fail(ctx, KNERF_ERR_INVALID, "wgrad_group_gb: >= 0");
        ctx->wgrad_group_gb = value; ctx->group_cache = 0;
    } else if (n.rfind("wgrad_cost", 0) == 0 && n.size() >= 11 && n.size() <= 12 && std::atoi(n.c_str() + 10) < ctx->si.n_jobs && n[10] >= '0' && n[10] <= '9') {
        if (value < 0 || value > 1e6) return fail(ctx, KNERF_ERR_INVALID, "wgrad_cost: 0..1e6");
        ctx->wgrad_cost[std::atoi(n.c_str() + 10)] = (int)value; ctx->plan_dirty = true;
    } else {
        return fail(ctx, KNERF_ERR_INVALID, "unknown option '" + n + "'");
    }
    return KNERF_OK;
}

int knerf_get_option(knerf_ctx* ctx, const char* name, double* value) {
    if (!ctx || !name || !value) return KNERF_ERR_INVALID;
    const std::string n(name);
    if (n == "deterministic") *value = ctx->deterministic;
    else if (n == "skip_dead_tiles") *value = ctx->skip_dead;
    else if (n == "grad_diagnostics") *value = ctx->grad_diag;
    else if (n == "occupancy_train") *value = ctx->occ_train;
    else if (n == "termination_threshold") *value = ctx->term_eps;
    else if (n == "termination_segment") *value = ctx->term_L;
    else if (n == "skip_dead_tiles_active") *value = skipping(ctx);
    else if (n == "wgrad_group_max") *value = ctx->wgrad_group_max;
    else if (n == "merge_chunk_rays") *value = ctx->merge_rays;
    else if (n == "merge_render_rays") *value = ctx->merge_render_rays;
    else if (n == "workspace_limit_gb") *value = ctx->ws_limit_gb;
    else if (n == "merge_fallbacks") *value = ctx->merge_fallbacks;
    else if (n == "wgrad_group_gb") *value = ctx->wgrad_group_gb;
    else if (n == "wgrad_group") *value = ctx->ws_train ? ctx->ws_group : 0;            // chunks per coarse wgrad launch of the current workspaces
    else if (n == "general_shape_path") *value = ctx->generic;
    else if (n.rfind("wgrad_cost", 0) == 0 && n.size() >= 11 && n.size() <= 12 && n[10] >= '0' && n[10] <= '9' && std::atoi(n.c_str() + 10) < ctx->si.n_jobs)
        *value = ctx->wgrad_cost[std::atoi(n.c_str() + 10)];
    else return fail(ctx, KNERF_ERR_INVALID, "unknown option '" + n + "'");
    return KNERF_OK;
}

int knerf_tile_stats_net(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset) {
    long long h[8];
    if (int r = read_stats(ctx, stream, &knerf_ctx::tile_stats, live, total, reset, h)) return r;
    if (h[2] || h[3] || h[6] || h[7])      // only a -DKNERF_LIST_GUARD build counts these
        return fail(ctx, KNERF_ERR_HIP, "tile list held " + std::to_string(h[2] + h[6]) + " (dgrad) / " + std::to_string(h[3] + h[7]) + " (wgrad) entries outside their pass");
    return KNERF_OK;
}

int knerf_tile_stats(knerf_ctx* ctx, void* stream, int64_t* live, int64_t* total, int reset) {
    if (!ctx || !live || !total) return KNERF_ERR_INVALID;
    int64_t l[2], t[2];
    const int r = knerf_tile_stats_net(ctx, stream, l, t, reset);
    *live = l[0] + l[1]; *total = t[0] + t[1];
    return r;
}

int knerf_grad_diagnostics(knerf_ctx* ctx, void* stream, int wait, int64_t* out) {
    if (!ctx || !out) return KNERF_ERR_INVALID;
    if (wait) HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    // seqlock reader (optim.hip diag_publish_kernel): [2] = published, [3] = begun.  Equal on both sides of the reads <=> the two
    // counts belong to step [2]; a publication in flight makes them differ for a few microseconds.
    volatile long long* h = ctx->h_diag;
    for (int attempt = 0; attempt < 4096; ++attempt) {
        const long long done = h[2];
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const long long c = h[0], f = h[1];
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const long long begun = h[3];
        if (begun == done) { out[0] = c; out[1] = f; out[2] = done; return KNERF_OK; }
    }
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));       // never seen in practice: settle it the slow way
    out[2] = h[2]; out[0] = h[0]; out[1] = h[1];
    return KNERF_OK;
}

int knerf_step_count(const knerf_ctx* ctx) { return ctx ? ctx->step : KNERF_ERR_INVALID; }
int knerf_set_step_count(knerf_ctx* ctx, int step) {
    if (!ctx || step < 0) return KNERF_ERR_INVALID;
    HIPCHK(hipDeviceSynchronize());        // steps still in flight count from the old value
    ctx->step = step;
    if (ctx->opt_ext) HIPCHK(launch_step_set_ext(step, ctx->d_step, ctx->d_lr_t, ctx->opt.weight_decay > 0 ? ctx->d_opt_f : nullptr, sched_args(ctx), nullptr));
    else HIPCHK(launch_step_set(step, ctx->d_step, ctx->d_lr_t, AdamHyper{ctx->cfg.lr, ctx->cfg.beta1, ctx->cfg.beta2}, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return KNERF_OK;
}

// validation and argument fill shared by each plain ray entry point and its _ext twin; `who` prefixes the messages
static int raygen_args(knerf_ctx* ctx, const char* who, const float* c2w, const float* noise, uint64_t seed, uint64_t stream_id, int batch, int height,
                       int width, int n_samples, float focal, float near_plane, float far_plane, float* o, float* d, float* t, RayGenArgs* out) {
    if (!c2w || !o || !d || !t || batch <= 0 || height <= 0 || width <= 0 || n_samples <= 0)
        return fail(ctx, KNERF_ERR_INVALID, std::string(who) + ": null/empty argument");
    RayGenArgs a{};
    a.c2w = c2w; a.noise = noise; a.o = o; a.d = d; a.t = t; a.B = batch; a.H = height; a.W = width; a.N = n_samples;
    a.focal = focal; a.near_ = near_plane; a.far_ = far_plane; a.seed = seed; a.stream_id = stream_id;
    *out = a;
    return KNERF_OK;
}

static int raybatch_args(knerf_ctx* ctx, const char* who, const float* images, const float* c2w, int n_views, int height, int width, int channels,
                         float focal, float near_plane, float far_plane, int n_samples, uint64_t seed, uint64_t epoch, uint64_t first, int n_rays,
                         const float* noise, uint64_t noise_stream, float* o, float* d, float* t, float* target, int64_t* index, RayBatchArgs* out) {
    const std::string w = std::string(who) + ": ";
    if (!images || !c2w || !o || !d || !t || !target || n_views <= 0 || height <= 0 || width <= 0 || n_samples <= 0 || n_rays <= 0)
        return fail(ctx, KNERF_ERR_INVALID, w + "null/empty argument");
    if (channels != 3 && channels != 4) return fail(ctx, KNERF_ERR_INVALID, w + "channels must be 3 or 4");
    const unsigned long long hw = (unsigned long long)height * (unsigned long long)width;
    if (hw >= (1ull << 31) || hw * (unsigned long long)n_views >= (1ull << 40))
        return fail(ctx, KNERF_ERR_INVALID, w + "the dataset must hold fewer than 2^40 pixels (2^31 per view)");
    const unsigned long long P = hw * (unsigned long long)n_views;
    if (first > P || (unsigned long long)n_rays > P - first)
        return fail(ctx, KNERF_ERR_INVALID, w + "first + n_rays exceeds the pixels of the dataset");
    if ((unsigned long long)n_rays * (unsigned long long)n_samples >= (1ull << 39))
        return fail(ctx, KNERF_ERR_INVALID, w + "n_rays x n_samples is too large for one launch");
    RayBatchArgs a{};
    a.images = images; a.c2w = c2w; a.noise = noise; a.o = o; a.d = d; a.t = t; a.target = target; a.index = (long long*)index;
    a.perm = make_pixel_perm(P, seed, epoch);
    a.first = first; a.seed = seed; a.noise_stream = noise_stream;
    a.n_rays = n_rays; a.H = height; a.W = width; a.C = channels; a.N = n_samples;
    a.focal = focal; a.near_ = near_plane; a.far_ = far_plane;
    *out = a;
    return KNERF_OK;
}

// the checks of a ray model against the sample range it is used with; null = pinhole rays with linear spacing
static int check_ray_model(knerf_ctx* ctx, const char* who, const knerf_ray_model* model, float near_plane, float far_plane, RayModel* out) {
    const std::string w = std::string(who) + ": ";
    knerf_ray_model m{0, KNERF_SPACING_LINEAR, 1.f};
    if (model) m = *model;
    if (m.ndc != 0 && m.ndc != 1) return fail(ctx, KNERF_ERR_INVALID, w + "ndc must be 0 or 1");
    if (m.spacing != KNERF_SPACING_LINEAR && m.spacing != KNERF_SPACING_DISPARITY)
        return fail(ctx, KNERF_ERR_INVALID, w + "unknown spacing " + std::to_string(m.spacing));
    if (!(std::isfinite(m.ndc_near) && m.ndc_near > 0.f)) return fail(ctx, KNERF_ERR_INVALID, w + "ndc_near must be finite and > 0");
    if (m.ndc && m.spacing == KNERF_SPACING_DISPARITY)
        return fail(ctx, KNERF_ERR_INVALID, w + "NDC rays are sampled linearly in NDC depth; disparity spacing is for pinhole rays");
    if (m.spacing == KNERF_SPACING_DISPARITY && !(near_plane > 0.f && far_plane > 0.f))
        return fail(ctx, KNERF_ERR_INVALID, w + "disparity spacing needs near_plane > 0");
    if (m.ndc && !(near_plane >= 0.f && far_plane <= 1.f && near_plane <= far_plane))
        return fail(ctx, KNERF_ERR_INVALID, w + "NDC rays take their samples at fractions of the ray: need 0 <= near_plane <= far_plane <= 1");
    *out = RayModel{m.ndc, m.spacing, m.ndc_near};
    return KNERF_OK;
}

int knerf_generate_rays(knerf_ctx* ctx, void* stream, const float* c2w, const float* noise, uint64_t seed, uint64_t stream_id,
                        int batch, int height, int width, int n_samples, float focal, float near_plane, float far_plane,
                        float* o, float* d, float* t) {
    RayGenArgs a{};
    if (int r = raygen_args(ctx, "generate_rays", c2w, noise, seed, stream_id, batch, height, width, n_samples, focal, near_plane, far_plane, o, d, t, &a)) return r;
    if (launch_raygen(a, (hipStream_t)stream) != hipSuccess) return fail(ctx, KNERF_ERR_HIP, "generate_rays: launch failed");
    return KNERF_OK;
}

int knerf_generate_rays_ext(knerf_ctx* ctx, void* stream, const float* c2w, const float* noise, uint64_t seed, uint64_t stream_id,
                            int batch, int height, int width, int n_samples, float focal, float near_plane, float far_plane,
                            float* o, float* d, float* t, const knerf_ray_model* model) {
    RayGenArgs a{};
    if (int r = raygen_args(ctx, "generate_rays_ext", c2w, noise, seed, stream_id, batch, height, width, n_samples, focal, near_plane, far_plane, o, d, t, &a)) return r;
    if ((unsigned long long)batch * (unsigned long long)height * (unsigned long long)width >= (1ull << 39) / (unsigned long long)n_samples)
        return fail(ctx, KNERF_ERR_INVALID, "generate_rays_ext: batch x height x width x n_samples is too large for one launch");
    RayModel m{};
    if (int r = check_ray_model(ctx, "generate_rays_ext", model, near_plane, far_plane, &m)) return r;
    if (launch_raygen_ext(a, m, (hipStream_t)stream) != hipSuccess) return fail(ctx, KNERF_ERR_HIP, "generate_rays_ext: launch failed");
    return KNERF_OK;
}

int knerf_draw_ray_batch(knerf_ctx* ctx, void* stream, const float* images, const float* c2w, int n_views, int height, int width,
                         int channels, float focal, float near_plane, float far_plane, int n_samples, uint64_t seed, uint64_t epoch,
                         uint64_t first, int n_rays, const float* noise, uint64_t noise_stream, float* o, float* d, float* t,
                         float* target, int64_t* index) {
    RayBatchArgs a{};
    if (int r = raybatch_args(ctx, "draw_ray_batch", images, c2w, n_views, height, width, channels, focal, near_plane, far_plane, n_samples, seed, epoch,
                              first, n_rays, noise, noise_stream, o, d, t, target, index, &a)) return r;
    if (launch_raybatch(a, (hipStream_t)stream) != hipSuccess) return fail(ctx, KNERF_ERR_HIP, "draw_ray_batch: launch failed");
    return KNERF_OK;
}

int knerf_draw_ray_batch_ext(knerf_ctx* ctx, void* stream, const float* images, const float* c2w, int n_views, int height, int width,
                             int channels, float focal, float near_plane, float far_plane, int n_samples, uint64_t seed, uint64_t epoch,
                             uint64_t first, int n_rays, const float* noise, uint64_t noise_stream, float* o, float* d, float* t,
                             float* target, int64_t* index, const knerf_ray_model* model) {
    RayBatchArgs a{};
    if (int r = raybatch_args(ctx, "draw_ray_batch_ext", images, c2w, n_views, height, width, channels, focal, near_plane, far_plane, n_samples, seed, epoch,
                              first, n_rays, noise, noise_stream, o, d, t, target, index, &a)) return r;
    RayModel m{};
    if (int r = check_ray_model(ctx, "draw_ray_batch_ext", model, near_plane, far_plane, &m)) return r;
    if (launch_raybatch_ext(a, m, (hipStream_t)stream) != hipSuccess) return fail(ctx, KNERF_ERR_HIP, "draw_ray_batch_ext: launch failed");
    return KNERF_OK;
}

// ---- camera models (include/knerf.h knerf_generate_rays_cam; rays_cam.h) -----------------------------------------------------------
// the checks of a camera against the views of the call and the ray model it is used with; the table's values stay unread (device)
static int check_camera(knerf_ctx* ctx, const char* who, const float* intrinsics, int n_cameras, const knerf_camera_model* camera,
                        int views, const RayModel* m, CamArgs* out) {
    const std::string w = std::string(who) + ": ";
    if (!camera || !intrinsics) return fail(ctx, KNERF_ERR_INVALID, w + "null camera or intrinsics");
    if (camera->model != KNERF_CAMERA_PINHOLE && camera->model != KNERF_CAMERA_OPENCV && camera->model != KNERF_CAMERA_FISHEYE)
        return fail(ctx, KNERF_ERR_INVALID, w + "unknown camera model " + std::to_string(camera->model));
    if (!std::isfinite(camera->pixel_offset)) return fail(ctx, KNERF_ERR_INVALID, w + "pixel_offset must be finite");
    if (n_cameras != 1 && (views <= 0 || n_cameras != views))
        return fail(ctx, KNERF_ERR_INVALID, w + "n_cameras must be 1 or the number of views (" + std::to_string(views) + "), got " + std::to_string(n_cameras));
    if (m && m->ndc && camera->model == KNERF_CAMERA_FISHEYE)
        return fail(ctx, KNERF_ERR_INVALID, w + "NDC rays need a camera that looks along -z: not the fisheye model");
    if (m && m->ndc && n_cameras > 1)
        return fail(ctx, KNERF_ERR_INVALID, w + "NDC rays take their scales from one camera: n_cameras must be 1");
    *out = CamArgs{intrinsics, n_cameras > 1 ? 1 : 0, camera->pixel_offset};
    return KNERF_OK;
}

int knerf_generate_rays_cam(knerf_ctx* ctx, void* stream, const float* c2w, const float* noise, uint64_t seed, uint64_t stream_id,
                            int batch, int height, int width, int n_samples, const float* intrinsics, int n_cameras,
                            const knerf_camera_model* camera, float near_plane, float far_plane, float* o, float* d, float* t,
                            const knerf_ray_model* model) {
    RayGenArgs a{};
    if (int r = raygen_args(ctx, "generate_rays_cam", c2w, noise, seed, stream_id, batch, height, width, n_samples, 0.f, near_plane, far_plane, o, d, t, &a)) return r;
    if ((unsigned long long)batch * (unsigned long long)height * (unsigned long long)width >= (1ull << 39) / (unsigned long long)n_samples)
        return fail(ctx, KNERF_ERR_INVALID, "generate_rays_cam: batch x height x width x n_samples is too large for one launch");
    RayModel m{};
    if (int r = check_ray_model(ctx, "generate_rays_cam", model, near_plane, far_plane, &m)) return r;
    CamArgs c{};
    if (int r = check_camera(ctx, "generate_rays_cam", intrinsics, n_cameras, camera, batch, &m, &c)) return r;
    if (launch_raygen_cam(a, m, c, camera->model, (hipStream_t)stream) != hipSuccess) return fail(ctx, KNERF_ERR_HIP, "generate_rays_cam: launch failed");
    return KNERF_OK;
}

int knerf_draw_ray_batch_cam(knerf_ctx* ctx, void* stream, const float* images, const float* c2w, int n_views, int height, int width,
                             int channels, const float* intrinsics, int n_cameras, const knerf_camera_model* camera, float near_plane,
                             float far_plane, int n_samples, uint64_t seed, uint64_t epoch, uint64_t first, int n_rays,
                             const float* noise, uint64_t noise_stream, float* o, float* d, float* t, float* target, int64_t* index,
                             const knerf_ray_model* model) {
    RayBatchArgs a{};
    if (int r = raybatch_args(ctx, "draw_ray_batch_cam", images, c2w, n_views, height, width, channels, 0.f, near_plane, far_plane, n_samples, seed, epoch,
                              first, n_rays, noise, noise_stream, o, d, t, target, index, &a)) return r;
    RayModel m{};
    if (int r = check_ray_model(ctx, "draw_ray_batch_cam", model, near_plane, far_plane, &m)) return r;
    CamArgs c{};
    if (int r = check_camera(ctx, "draw_ray_batch_cam", intrinsics, n_cameras, camera, n_views, &m, &c)) return r;
    if (launch_raybatch_cam(a, m, c, camera->model, (hipStream_t)stream) != hipSuccess) return fail(ctx, KNERF_ERR_HIP, "draw_ray_batch_cam: launch failed");
    return KNERF_OK;
}

int knerf_project_points(void* stream, const float* points, const int32_t* view, const float* c2w, const float* intrinsics, int n_cameras,
                         const knerf_camera_model* camera, uint64_t n, float* pixels, float* depth, uint8_t* valid) {
    if (!points || !c2w || !pixels || !depth || !valid || n == 0) return fail(nullptr, KNERF_ERR_INVALID, "project_points: null/empty argument");
    if (n >= (1ull << 39)) return fail(nullptr, KNERF_ERR_INVALID, "project_points: too many points for one launch");
    if (n_cameras < 1) return fail(nullptr, KNERF_ERR_INVALID, "project_points: n_cameras must be at least 1");
    CamArgs c{};
    if (int r = check_camera(nullptr, "project_points", intrinsics, n_cameras, camera, n_cameras, nullptr, &c)) return r;
    ProjectArgs a{points, (const int*)view, c2w, c, (unsigned long long)n, pixels, depth, (unsigned char*)valid};
    if (launch_project_points(a, camera->model, (hipStream_t)stream) != hipSuccess) return fail(nullptr, KNERF_ERR_HIP, "project_points: launch failed");
    return KNERF_OK;
}

int knerf_profile_enable(knerf_ctx* ctx, int on) {
    if (!ctx) return KNERF_ERR_INVALID;
    ctx->prof_on = on != 0;
    return KNERF_OK;
}

int knerf_profile_read(knerf_ctx* ctx, double* total_ms, int64_t* launches, int n) {
    if (!ctx || !total_ms || !launches || n < P_COUNT) return KNERF_ERR_INVALID;
    for (int i = 0; i < n; ++i) { total_ms[i] = 0.0; launches[i] = 0; }
    HIPCHK(hipDeviceSynchronize());
    for (auto& r : ctx->prof) {
        float ms = 0.f;
        if (r.e0 && r.e1 && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { total_ms[r.id] += ms; launches[r.id] += 1; }
        if (r.e0) (void)hipEventDestroy(r.e0);
        if (r.e1) (void)hipEventDestroy(r.e1);
    }
    ctx->prof.clear();
    return KNERF_OK;
}

}  // extern "C"
