// debug_api.hip -- diagnostics behind include/knerf_debug.h (libknerf_probe.so; tests/ and tools/ only, never the product).
#include <cstring>
#include <vector>

#include "../../include/knerf_debug.h"
#include "composite_ext.h"
#include "ctx.h"
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
