// debug_api.hip -- diagnostics behind include/knerf_debug.h (libknerf_probe.so; tests/ and tools/ only, never the product).
#include <cstring>
#include <vector>

#include "../../include/knerf_debug.h"
#include "composite_ext.h"
#include "ctx.h"
#include "generic.h"
#include "kernels.h"

using namespace knerf;

extern "C" {

int knerf_debug_generic_plan(const knerf_config* cfg, int32_t* out, size_t* n) {
    if (!cfg || !n || knerf_param_count_for(cfg) == 0) return KNERF_ERR_INVALID;
    const gen::Plan p = gen::build_plan(cfg->n_layers, cfg->dense_units, cfg->skip_layer, cfg->pos_emb_xyz, cfg->pos_emb_dir);
    std::vector<int32_t> v;
    auto r32 = [](int v) { return (v + 31) / 32 * 32; };
    for (size_t li = 0; li < p.layers.size(); ++li) {
        const gen::Layer& L = p.layers[li];
        // padded input width: the buffer's ld for the trunk layers; the four head layers are evaluated together on the composed
        // matrix (generic.h) and own no buffer, so theirs is the width a stand-alone layer would have
        const int in_ld = (int)li < p.n_layers ? p.buf_ld[L.in_buf] : r32(L.seg[0].width) + (L.n_seg == 2 ? r32(L.seg[1].width) : 0);
        const int32_t row[16] = {L.w_off, L.b_off, L.k_real, L.n_real, in_ld, L.np, L.n_seg, L.seg[0].col0, L.seg[0].width,
                                 L.seg[0].wrow0, L.seg[1].col0, L.seg[1].width, L.seg[1].wrow0, L.relu, L.head, L.out_buf < 0 ? -1 : p.buf_ld[L.out_buf]};
        v.insert(v.end(), row, row + 16);
    }
    if (out) {
        if (*n < v.size()) return KNERF_ERR_INVALID;
        memcpy(out, v.data(), v.size() * sizeof(int32_t));
    }
    *n = v.size();
    return KNERF_OK;
}

int knerf_debug_table(int kind, int32_t* out, size_t* n) {
    if (!n || kind < 0) return KNERF_ERR_INVALID;
    const int shape = kind >> 4;        // kind + 16 * (index in csrc/layout.h KNERF_FUSED_SHAPES); kind 5: {n_layers, skip_layer, dense_units, param_count, pos_emb_xyz, pos_emb_dir} of that shape
    kind &= 15;
    if (shape >= kNumFusedShapes) return KNERF_ERR_INVALID;
    const Tables& t = host_tables(shape);
    const ShapeInfo& si = shape_info(shape);
    const std::vector<int32_t> info = {si.n_layers, si.skip, si.units, si.param_count, si.lx, si.ld};
    const std::vector<int32_t>* v = nullptr;
    switch (kind) {
        case 5: v = &info; break;
        case 0: v = &t.host.fwd; break;
        case 1: v = &t.host.fwd_bias; break;
        case 2: v = &t.host.bwd; break;
        case 3: v = &t.wgrad; break;
        case 4: v = &t.wgrad_off; break;
        default: return KNERF_ERR_INVALID;
    }
    if (out) {
        if (*n < v->size()) return KNERF_ERR_INVALID;
        memcpy(out, v->data(), v->size() * sizeof(int32_t));
    }
    *n = v->size();
    return KNERF_OK;
}

int knerf_debug_buffer(knerf_ctx* ctx, int net, int which, void** dev, size_t* bytes) {
    if (!ctx || !dev || !bytes) return KNERF_ERR_INVALID;
    auto view = [&](const auto& b) { *dev = b.get(); *bytes = b.bytes(); };
    switch (which) {
        case 0: view(ctx->act); break;
        case 1: view(ctx->mask); break;
        case 2: view(ctx->dz); break;
        case 3: view(ctx->raw); break;
        case 4: view(ctx->draw); break;      // sized by the largest TRAINING chunk (raw follows renders too)
        case 5: view(ctx->t_f); break;
        case 6: view(ctx->w_c); break;
        case 7:
            if (net != 0 && net != 1) return KNERF_ERR_INVALID;
            view(ctx->net[net].w); break;
        // general-shape path (generic.h): every activation buffer [Mp][ld] bf16 / every dZ buffer of the last pass
        case 8: view(ctx->gws_buf.act); break;
        case 9: view(ctx->gws_buf.dz); break;
        default: return KNERF_ERR_INVALID;
    }
    // not allocated: no pass has run yet, or the buffer belongs to the fused path and this context runs the general-shape kernels
    return *dev ? KNERF_OK : KNERF_ERR_INVALID;
}

int knerf_debug_composite_train(void* stream, const float* raw, const float* t, const float* target, int n_rays, int n_samples,
                                int white_background, float grad_scale, float loss_scale, float* image, float* depth, float* weights,
                                float* draw, float* loss, float* loss_partial, int* tile_flags, int* tile_list, int* tile_count,
                                int* tile_list2, int* tile_count2, int tile_off2) {
    if (!raw || !t || !target || !image || !depth || !weights || !draw || !loss || n_rays <= 0 || n_samples <= 0 || n_samples > 1024)
        return KNERF_ERR_INVALID;
    if ((tile_flags || tile_list) && n_samples % 32 != 0) return KNERF_ERR_INVALID;          // tiles must not straddle rays
    if (!tile_list != !tile_count || !tile_list2 != !tile_count2 || (tile_list2 && !tile_list)) return KNERF_ERR_INVALID;
    CompositeArgs ca{};
    ca.raw = raw; ca.t = t; ca.target = target; ca.image = image; ca.depth = depth; ca.weights = weights;
    ca.draw = draw; ca.loss = loss; ca.R = n_rays; ca.S = n_samples; ca.white = white_background;
    ca.grad_scale = grad_scale; ca.loss_scale = loss_scale;
    ca.tile_flags = tile_flags; ca.tile_list = tile_list; ca.tile_count = tile_count;
    ca.tile_list2 = tile_list2; ca.tile_count2 = tile_count2; ca.tile_off2 = tile_off2;
    ca.loss_partial = loss_partial;
    hipStream_t s = (hipStream_t)stream;
    if (launch_composite(ca, s) != hipSuccess) return KNERF_ERR_HIP;
    // deterministic mode, as knerf_train_chunk: the workgroups' loss terms added in a fixed order
    if (ca.loss_partial && launch_loss_reduce(ca.loss_partial, (n_rays + 3) / 4, loss, s) != hipSuccess) return KNERF_ERR_HIP;
    return KNERF_OK;
}

int knerf_debug_composite_objective(void* stream, const float* raw, const float* t, const float* target, int n_rays, int n_samples,
                                    int white_background, float grad_scale, float loss_scale, float* image, float* depth, float* weights,
                                    float* draw, float* loss, float* loss_partial, int* tile_flags, int* tile_list, int* tile_count,
                                    int* tile_list2, int* tile_count2, int tile_off2, const knerf_objective* obj, float reg_scale,
                                    float* terms, float* terms_partial) {
    if (!raw || !t || !target || !image || !depth || !weights || !draw || !loss || n_rays <= 0 || n_samples <= 0 || n_samples > 1024)
        return KNERF_ERR_INVALID;
    if ((tile_flags || tile_list) && n_samples % 32 != 0) return KNERF_ERR_INVALID;
    if (!tile_list != !tile_count || !tile_list2 != !tile_count2 || (tile_list2 && !tile_list)) return KNERF_ERR_INVALID;
    if (!obj || !terms || !loss_partial != !terms_partial) return KNERF_ERR_INVALID;
    if (obj->loss_kind < KNERF_LOSS_MSE || obj->loss_kind > KNERF_LOSS_LOG_COSH || (obj->loss_kind == KNERF_LOSS_HUBER && !(obj->huber_delta > 0)))
        return KNERF_ERR_INVALID;
    CompositeArgs ca{};
    ca.raw = raw; ca.t = t; ca.target = target; ca.image = image; ca.depth = depth; ca.weights = weights;
    ca.draw = draw; ca.loss = loss; ca.R = n_rays; ca.S = n_samples; ca.white = white_background;
    ca.grad_scale = grad_scale; ca.loss_scale = loss_scale;
    ca.tile_flags = tile_flags; ca.tile_list = tile_list; ca.tile_count = tile_count;
    ca.tile_list2 = tile_list2; ca.tile_count2 = tile_count2; ca.tile_off2 = tile_off2;
    ca.loss_partial = loss_partial;
    // always the extended kernel, also for mse without a regulariser (the product takes the plain kernel there)
    CompositeExt ce{};
    ce.loss_kind = obj->loss_kind; ce.huber_delta = obj->huber_delta; ce.lambda_d = obj->distortion; ce.lambda_e = obj->opacity_entropy;
    ce.reg_scale = reg_scale; ce.terms = terms; ce.terms_partial = terms_partial;
    hipStream_t s = (hipStream_t)stream;
    if (launch_composite(ca, &ce, s) != hipSuccess) return KNERF_ERR_HIP;
    if (ca.loss_partial && launch_loss_reduce(ca.loss_partial, (n_rays + 3) / 4, loss, s) != hipSuccess) return KNERF_ERR_HIP;
    if (ce.terms_partial && launch_terms_reduce(ce.terms_partial, (n_rays + 3) / 4, terms, s) != hipSuccess) return KNERF_ERR_HIP;
    return KNERF_OK;
}

int knerf_debug_compact_tiles(const int* flags, int n, int period, int real, int* list, int* count, long long* stats, void* stream) {
    if (!flags || !list || !count || n <= 0 || period <= 0 || real < 0 || real > period) return KNERF_ERR_INVALID;
    return launch_compact_tiles(flags, n, period, real, list, count, stats, (hipStream_t)stream) == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

}  // extern "C"

// ---- the general-shape path's matmul launchers on caller-made buffers ----------------------------------------------------
// Everything the kernels will address is checked here, on the host, before the first HIP call: these kernels take raw pointers.
namespace {
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the live-tile list: host entries in [0, tiles), strictly ascending where asked; uploaded as {count, entries...} into dev
bool live_ok(const int32_t* live, long long n_live, long long tiles, bool ascending, const int32_t* dev, size_t dev_elems) {
    if (!live && n_live < 0) return true;                       // no list
    if (n_live < 0 || n_live > tiles || (!live && n_live > 0) || !dev || dev_elems < (size_t)n_live + 1 || ((uintptr_t)dev & 3)) return false;
    for (long long i = 0; i < n_live; ++i) {
        if (live[i] < 0 || live[i] >= tiles) return false;
        if (ascending && i > 0 && live[i] <= live[i - 1]) return false;
    }
    return true;
}
int live_upload(const int32_t* live, long long n_live, int32_t* dev, hipStream_t s) {
    const int32_t cnt = (int32_t)n_live;
    if (hipMemcpyAsync(dev, &cnt, sizeof(cnt), hipMemcpyHostToDevice, s) != hipSuccess) return KNERF_ERR_HIP;
    if (n_live > 0 && hipMemcpyAsync(dev + 1, live, (size_t)n_live * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess) return KNERF_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;     // the host copies may go out of scope
}

int check_gemm(const knerf_debug_gemm* a) {
    if (!a) return KNERF_ERR_INVALID;
    const long long M = a->M;
    const int N = a->N, K = a->K;
    if (M <= 0 || M % 128 || M > (1ll << 24) || N <= 0 || N % 32 || N > 4096 || K <= 0 || K % 32 || K > 8192) return KNERF_ERR_INVALID;
    const gen::GemmLaunch d = gen::describe_gemm(M, N, K);
    const size_t rows = (size_t)M;
    // operands: 16-byte loads of 8 elements
    if (!a->A || !a->Bt || !aligned16(a->A) || !aligned16(a->Bt)) return KNERF_ERR_INVALID;
    if (a->lda < K || a->ldb < K || a->lda % 8 || a->ldb % 8) return KNERF_ERR_INVALID;
    if (a->a_elems < (rows - 1) * a->lda + K || a->bt_elems < (size_t)(N - 1) * a->ldb + K) return KNERF_ERR_INVALID;
    if (a->bias && (a->n_real < 0 || a->n_real > N || a->bias_elems < (size_t)a->n_real || ((uintptr_t)a->bias & 3))) return KNERF_ERR_INVALID;
    // exactly one output; the relu bits go with the bf16 one, written or read, never both
    if (!a->Cb == !a->Cf) return KNERF_ERR_INVALID;
    if (a->mask_out && a->mask_in) return KNERF_ERR_INVALID;
    if (a->Cf) {
        if (a->mask_out || a->mask_in || a->relu || ((uintptr_t)a->Cf & 3) || a->ldcf < N || a->cf_elems < (rows - 1) * a->ldcf + N) return KNERF_ERR_INVALID;
    } else {
        // a lane stores its nt consecutive features of a row as ONE 2 nt-byte access
        if (!aligned16(a->Cb) || a->c_col0 < 0 || a->c_col0 % d.nt || a->ldc % d.nt || a->ldc < a->c_col0 + N) return KNERF_ERR_INVALID;
        if (a->cb_elems < (rows - 1) * a->ldc + a->c_col0 + N) return KNERF_ERR_INVALID;
    }
    if (a->mask_in && (a->bias || a->relu)) return KNERF_ERR_INVALID;           // the dgrad form has neither
    const unsigned char* mk = a->mask_out ? a->mask_out : a->mask_in;
    if (mk && (!aligned16(mk) || a->mask_cols < N / 8 || a->mask_bytes < (size_t)(M / 32) * a->mask_cols * 32)) return KNERF_ERR_INVALID;
    if (!live_ok(a->live, a->n_live, M / 32, false, a->live_dev, a->live_dev_elems)) return KNERF_ERR_INVALID;

    return KNERF_OK;
}

int check_wgrad(const knerf_debug_wgrad* a) {
    if (!a) return KNERF_ERR_INVALID;
    const long long steps = a->steps;
    const int N = a->N, K = a->K;
    if (steps <= 0 || steps > (1ll << 19) || N <= 0 || N % 32 || N > 4096 || K <= 0 || K % 32 || K > 8192) return KNERF_ERR_INVALID;
    if (a->selector != 0 && a->selector != 1) return KNERF_ERR_INVALID;
    const size_t rows = (size_t)steps * 32;
    // operands: 16-byte loads (LDS-DMA or registers) of 8 elements
    if (!a->X || !a->Z || !aligned16(a->X) || !aligned16(a->Z)) return KNERF_ERR_INVALID;
    if (a->ldx < K || a->ldz < N || a->ldx % 8 || a->ldz % 8) return KNERF_ERR_INVALID;
    if (a->x_elems < (rows - 1) * a->ldx + K || a->z_elems < (rows - 1) * a->ldz + N) return KNERF_ERR_INVALID;
    // destinations: kernel rows of every segment and the bias, inside the gradient
    if (!a->grad || ((uintptr_t)a->grad & 3) || a->n_real <= 0 || a->n_real > N || a->w_off < 0 || a->b_off < 0) return KNERF_ERR_INVALID;
    if (a->n_seg < 1 || a->n_seg > 2) return KNERF_ERR_INVALID;
    for (int i = 0; i < a->n_seg; ++i) {
        const int c0 = a->seg[3 * i], w = a->seg[3 * i + 1], r0 = a->seg[3 * i + 2];
        if (c0 < 0 || w <= 0 || r0 < 0 || c0 > K - w) return KNERF_ERR_INVALID;
        if (i == 1 && c0 < a->seg[0] + a->seg[1]) return KNERF_ERR_INVALID;                       // ascending, no shared column
        const size_t lo = (size_t)a->w_off + (size_t)r0 * a->n_real, hi = lo + (size_t)w * a->n_real;
        if (hi > a->grad_elems) return KNERF_ERR_INVALID;
        if (lo < (size_t)a->b_off + a->n_real && (size_t)a->b_off < hi) return KNERF_ERR_INVALID;      // the bias lies apart from the kernel
    }
    if ((size_t)a->b_off + a->n_real > a->grad_elems) return KNERF_ERR_INVALID;
    if (a->partial && (((uintptr_t)a->partial & 3) || a->partial_elems < gen::wgrad_partial_floats_for(K, N, a->selector))) return KNERF_ERR_INVALID;
    if (!live_ok(a->live, a->n_live, steps, a->partial != nullptr, a->live_dev, a->live_dev_elems)) return KNERF_ERR_INVALID;

    return KNERF_OK;
}
}  // namespace

extern "C" {

int knerf_debug_generic_launch(int what, long long m_or_steps, int N, int K, int per_wave, int32_t out[8]) {
    if (!out || m_or_steps <= 0 || N <= 0 || K <= 0 || N % 32 || K % 32) return KNERF_ERR_INVALID;
    if (what == 0) {
        if (m_or_steps % 32) return KNERF_ERR_INVALID;
        const gen::GemmLaunch d = gen::describe_gemm(m_or_steps, N, K);
        const int32_t v[8] = {d.ws, d.nt, d.gx, d.gy, (int32_t)d.lds, d.pitch, 0, 0};
        memcpy(out, v, sizeof(v));
        return KNERF_OK;
    }
    if (what == 1) {
        const gen::WgradLaunch d = gen::describe_wgrad(K, N, m_or_steps, per_wave);
        const int32_t v[8] = {d.coop, d.gx, d.gy, d.gz, d.kt, d.nt, d.n_slabs, (int32_t)d.slab_floats};
        memcpy(out, v, sizeof(v));
        return KNERF_OK;
    }
    return KNERF_ERR_INVALID;
}

int knerf_debug_generic_wgrad_partial_floats(int K, int N, int per_wave, size_t* floats) {
    if (!floats || N <= 0 || K <= 0 || N % 32 || K % 32) return KNERF_ERR_INVALID;
    *floats = gen::wgrad_partial_floats_for(K, N, per_wave);
    return KNERF_OK;
}

int knerf_debug_generic_check(int what, const void* args) {
    if (what == 0) return check_gemm((const knerf_debug_gemm*)args);
    if (what == 1) return check_wgrad((const knerf_debug_wgrad*)args);
    return KNERF_ERR_INVALID;
}

int knerf_debug_generic_gemm(void* stream, const knerf_debug_gemm* a) {
    if (check_gemm(a) != KNERF_OK) return KNERF_ERR_INVALID;
    const long long M = a->M;
    const int N = a->N, K = a->K;
    hipStream_t s = (hipStream_t)stream;
    const bool list = a->n_live >= 0;
    if (list) { const int rc = live_upload(a->live, a->n_live, a->live_dev, s); if (rc != KNERF_OK) return rc; }
    gen::GemmArgs g{};
    g.A = a->A; g.lda = a->lda; g.Bt = a->Bt; g.ldb = a->ldb; g.M = M; g.N = N; g.K = K;
    g.bias = a->bias; g.n_real = a->n_real; g.relu = a->relu;
    g.mask_out = a->mask_out; g.mask_in = a->mask_in; g.mask_cols = a->mask_cols;
    g.Cb = a->Cb ? a->Cb + a->c_col0 : nullptr; g.ldc = a->ldc; g.Cf = a->Cf; g.ldcf = a->ldcf;
    if (list) { g.live = a->live_dev + 1; g.n_live = a->live_dev; }
    return gen::launch_gemm(g, s) == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

int knerf_debug_generic_wgrad(void* stream, const knerf_debug_wgrad* a) {
    if (check_wgrad(a) != KNERF_OK) return KNERF_ERR_INVALID;
    const long long steps = a->steps;
    const int N = a->N, K = a->K;
    hipStream_t s = (hipStream_t)stream;
    const bool list = a->n_live >= 0;
    if (list) { const int rc = live_upload(a->live, a->n_live, a->live_dev, s); if (rc != KNERF_OK) return rc; }
    gen::WgradArgs w{};
    w.X = a->X; w.ldx = a->ldx; w.Z = a->Z; w.ldz = a->ldz; w.steps = steps; w.grad = a->grad;
    w.w_off = a->w_off; w.b_off = a->b_off; w.n_real = a->n_real; w.n_seg = a->n_seg;
    for (int i = 0; i < a->n_seg; ++i) w.seg[i] = gen::Seg{a->seg[3 * i], a->seg[3 * i + 1], a->seg[3 * i + 2]};
    w.partial = a->partial;
    if (list) { w.live = a->live_dev + 1; w.n_live = a->live_dev; }
    return gen::launch_wgrad(w, K, N, s, a->selector) == hipSuccess ? KNERF_OK : KNERF_ERR_HIP;
}

}  // extern "C"
