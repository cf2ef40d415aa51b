"""Training behind occupancy grids (option occupancy_train; csrc/train_list.hip, the compacted backward in knerf_api.hip run_pass) on the
GPU: with every cell occupied nothing changes (bit for bit in deterministic mode, at one chunk, merged chunks and a grouped coarse
weight-gradient launch, on two fused shapes); a random partial grid gives the gradients of the masked field (a NumPy oracle built from
oracle.nerf_oracle pieces), on the fused and the general-shape path alike; deterministic runs repeat bit for bit; the train stats count
what was skipped and leave the render stats alone; fit with OccupancyGridUpdater keeps the dense steps before its warm-up and trains
behind the grids afterwards."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import occupancy_reference as M
from tests.test_gpu_configs import GRAD_TOL_EMU
from tests.test_gpu_forward import log_stats
from tests.test_gpu_train import per_tensor_err

pytestmark = pytest.mark.gpu
LO, HI = (-1.5,) * 3, (1.5,) * 3
SHAPES = {"default": None, "l4_u128": O.NerfConfig(n_layers=4, skip_layer=2, dense_units=128)}


def _ctx(P, force_generic=False, **opts):
    from keras_nerf_amd.runtime import KnerfContext
    c = P["cfg"]
    ctx = KnerfContext(white_background=True, n_layers=c.n_layers, dense_units=c.dense_units, skip_layer=c.skip_layer,
                       pos_emb_xyz=c.pos_emb_xyz, pos_emb_dir=c.pos_emb_dir, force_generic=force_generic, options=opts or None)
    ctx.set_weights(0, O.flatten_params(P["cp"])); ctx.set_weights(1, O.flatten_params(P["fp"]))
    return ctx


def _grids(seed, cells=(16, 16, 16)):
    rng = np.random.default_rng(seed)
    return {0: rng.random(cells) < 0.5, 1: rng.random(cells[::-1]) < 0.5}


def _train(P, grids=None, ray_chunks=None, force_generic=False, **opts):
    """one train_batch + Adam: (losses, coarse image, fine image, coarse grads, fine grads, weights after Adam of both nets)"""
    from keras_nerf_amd.runtime import COARSE, FINE
    ctx = _ctx(P, force_generic=force_generic, **opts)
    if grids is not None:
        for net in (COARSE, FINE):
            ctx.set_occupancy(net, grids[net], LO, HI, "occupied")
        ctx.set_option("occupancy_train", 1)
    N = P["N"]
    o, d, t, u = (P[k].reshape(N, -1).astype(np.float32) for k in ("o", "d", "t", "u"))
    loss = torch.zeros(2, device="cuda")
    ci, fi = torch.empty((N, 3), device="cuda"), torch.empty((N, 3), device="cuda")
    ctx.train_batch(o, d, t, P["img"].reshape(N, 3), u, seed=1, ray_chunks=ray_chunks or N, loss=loss, c_image=ci, f_image=fi)
    g = (ctx.grads(0).clone(), ctx.grads(1).clone())
    group = ctx.get_option("wgrad_group")
    ctx.apply_adam()
    out = (loss.clone(), ci, fi, g[0], g[1], ctx.get_weights(0), ctx.get_weights(1))
    ctx.close()
    return out, group


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["single_chunk", "merged", "grouped"])
def test_all_occupied_is_bit_identical_to_dense(shape, mode):
    from tests.problem import make_problem
    P = make_problem(n_images=2, wh=16, weight_scale=1.5, bias_std=0.05, cfg=SHAPES[shape])
    kw = {"single_chunk": dict(ray_chunks=None), "merged": dict(ray_chunks=128),
          "grouped": dict(ray_chunks=128, merge_chunk_rays=0, wgrad_group_max=4)}[mode]
    full = {0: np.ones((8, 8, 8), bool), 1: np.ones((4, 5, 6), bool)}
    (dense, gd), (occ, go) = (_train(P, grids, deterministic=1, **kw) for grids in (None, full))
    assert gd == go and (gd > 1) == (mode == "grouped"), (gd, go)
    for i, (a, b) in enumerate(zip(dense, occ)):
        assert (torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(a, b)), (i, mode)
    # default mode: the same gradients up to the order of fp32 sums
    (dd, _), (oo, _) = (_train(P, grids, **kw) for grids in (None, full))
    for a, b in zip(dd[3:5], oo[3:5]):
        assert per_tensor_err(b.cpu().numpy(), a.cpu().numpy(), P["cfg"])[0] < 1e-4


def _masked_oracle(params, o, d, t, target, cfg, live, emulate):
    """loss and gradients of the masked field: raw = 0 at dead samples, and no dL/d(rgb, sigma) from them"""
    xyz, dire = O.encode_position_and_directions(o, d, t, cfg.pos_emb_xyz, cfg.pos_emb_dir)
    rgb, sigma, mc = O.mlp_forward(params, xyz, dire, cfg, emulate, True)
    rgb, sigma = rgb.copy(), sigma.copy()
    rgb[~live] = 0.0
    sigma[~live] = 0.0
    image, _, w, rc = O.render_image_depth_chunk(rgb, sigma, t, True, want_cache=True)
    dimg = (image.dtype.type(2.0) / image.dtype.type(image.size)) * (image - target)
    drgb, dsigma = O.render_backward(rc, dimg)
    drgb[~live] = 0.0
    dsigma[~live] = 0.0
    return float(O.mse(target, image)), O.flatten_params(O.mlp_backward(params, mc, drgb, dsigma, cfg)), image


def test_partial_grid_gives_the_masked_gradients():
    from keras_nerf_amd.runtime import COARSE, FINE
    from tests.problem import make_problem
    P = make_problem(n_images=1, wh=16, weight_scale=1.5, bias_std=0.05)
    cfg, N = P["cfg"], P["N"]
    o, d, t, u = (P[k].reshape(N, -1).astype(np.float32) for k in ("o", "d", "t", "u"))
    img = P["img"].reshape(N, 3)
    grids = _grids(21)
    # the fine pass's t-values: a render behind the same grids gives the coarse weights of the training pass, bit for bit
    r = _ctx(P)
    for net in (COARSE, FINE):
        r.set_occupancy(net, grids[net], LO, HI, "occupied")
    rend = r.render_chunk(o, d, t, u, seed=1)
    tf = rend["t_fine"].cpu().numpy()
    r.close()
    live_c = M.lookup(M.ray_points(o, d, t).reshape(-1, 3), grids[COARSE], LO, HI).reshape(N, -1)
    live_f = M.lookup(M.ray_points(o, d, tf).reshape(-1, 3), grids[FINE], LO, HI).reshape(N, -1)
    assert 0.1 < live_c.mean() < 0.9 and 0.1 < live_f.mean() < 0.9, (live_c.mean(), live_f.mean())
    n = O.param_count(cfg)
    ref, loss_ref = {}, {}
    for emulate in (O.FUSED, False):
        lc, gc, _ = _masked_oracle(P["cp"], o, d, t, img, cfg, live_c, emulate)
        lf, gf, _ = _masked_oracle(P["fp"], o, d, tf, img, cfg, live_f, emulate)
        ref[emulate], loss_ref[emulate] = (gc, gf), (lc, lf)
    _, gc_dense, _ = _masked_oracle(P["cp"], o, d, t, img, cfg, np.ones_like(live_c), O.FUSED)
    gap = [per_tensor_err(ref[O.FUSED][k], ref[False][k], cfg)[0] for k in (0, 1)]
    err, res = {}, {}
    for general in (False, True):
        out, _ = _train(P, grids, force_generic=general)
        res[general] = out
        if not general:
            assert torch.equal(out[1], rend["c_image"]), "the training pass's coarse image is the render's"
        g = (out[3].cpu().numpy()[:n], out[4].cpu().numpy()[:n])
        for emulate in (O.FUSED, False):
            err[general, emulate] = [per_tensor_err(g[k], ref[emulate][k], cfg)[0] for k in (0, 1)]
            for k in (0, 1):
                assert abs(float(out[0][k]) - loss_ref[emulate][k]) < 2e-3, (general, emulate, k)
        err[general, "dense"] = per_tensor_err(g[0], gc_dense, cfg)[0]
    fg = [per_tensor_err(res[True][k].cpu().numpy(), res[False][k].cpu().numpy(), cfg)[0] for k in (3, 4)]
    for (general, emulate), e in err.items():
        if emulate != "dense":
            log_stats(f"occupancy_train_masked_oracle_general{int(general)}_emulate{emulate}", coarse_worst=e[0], fine_worst=e[1])
    log_stats("occupancy_train_masked_oracle_gaps", bf16_vs_fp32_coarse=gap[0], bf16_vs_fp32_fine=gap[1], fused_vs_general_coarse=fg[0],
              fused_vs_general_fine=fg[1], fused_vs_dense_oracle=err[False, "dense"], general_vs_dense_oracle=err[True, "dense"])
    # measured on MI355X: fused vs the oracle in its own arithmetic 2.6e-2 (coarse, layer_1/kernel) / 3.9e-3 (fine); vs the fp32 oracle
    # 6.1e-2 / 1.06e-1 where the oracle's own bf16-vs-fp32 gap is 6.1e-2 / 1.06e-1; general path vs fp32 6.0e-2 / 9.0e-2; fused vs general
    # 2.6e-2 / 9.6e-2 (the general path's fine samples follow its own coarse weights); dense-field gradients 1.8 away
    assert max(err[False, O.FUSED]) < 3e-2, err
    # against the fp32 oracle, both paths: within the oracle's own bf16-vs-fp32 gap on this problem, plus the emulated tolerance
    for general in (False, True):
        for k in (0, 1):
            assert err[general, False][k] < gap[k] + GRAD_TOL_EMU, (general, k, err, gap)
    assert max(fg) < max(gap) + GRAD_TOL_EMU, (fg, gap)
    # the mask matters: training on the dense field gives other gradients
    assert err[False, "dense"] > 2 * GRAD_TOL_EMU and err[True, "dense"] > 2 * GRAD_TOL_EMU, err


def test_partial_grid_deterministic_runs_repeat():
    from tests.problem import make_problem
    P = make_problem(n_images=2, wh=16, weight_scale=1.5, bias_std=0.05)
    a, _ = _train(P, _grids(22), ray_chunks=128, deterministic=1, merge_chunk_rays=0, wgrad_group_max=2)
    b, _ = _train(P, _grids(22), ray_chunks=128, deterministic=1, merge_chunk_rays=0, wgrad_group_max=2)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y)), i


def test_train_stats_count_the_skipped_samples_and_leave_render_stats_alone():
    from keras_nerf_amd.runtime import COARSE, FINE
    from tests.problem import make_problem
    P = make_problem(n_images=1, wh=16, weight_scale=1.5, bias_std=0.05)
    N = P["N"]
    o, d, t, u = (P[k].reshape(N, -1).astype(np.float32) for k in ("o", "d", "t", "u"))
    ctx = _ctx(P)
    assert ctx.get_option("occupancy_train") == 0
    with pytest.raises(ValueError):
        ctx.set_option("occupancy_train", 2)
    g = _grids(23)
    for net in (COARSE, FINE):
        ctx.set_occupancy(net, g[net], LO, HI)
    ctx.occupancy_stats(reset=True); ctx.occupancy_train_stats(reset=True)
    ctx.train_batch(o, d, t, P["img"].reshape(N, 3), u, seed=1, ray_chunks=N)
    assert ctx.occupancy_train_stats() == ((0, 0), (0, 0))            # option off: dense, nothing counted
    ctx.set_option("occupancy_train", 1)
    ctx.train_batch(o, d, t, P["img"].reshape(N, 3), u, seed=1, ray_chunks=N)
    (lc, tc), (lf, tf) = ctx.occupancy_train_stats()
    assert 0 < lc < tc == N * 64 and 0 < lf < tf == N * 192, (lc, tc, lf, tf)
    live_c = M.lookup(M.ray_points(o, d, t).reshape(-1, 3), g[COARSE], LO, HI)
    assert lc == int(live_c.sum())
    assert ctx.occupancy_stats() == ((0, 0), (0, 0))                  # no render ran
    ctx.close()


def test_fit_with_the_grid_updater():
    """the compact procedural scene (density exactly 0 outside the objects): 160 dense steps, then grids every 16 steps"""
    from keras_nerf_amd.model.nerf.callback import OccupancyGridUpdater
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene
    wh, B, warm, steps = 32, 2, 160, 320
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=wh, n_views=24, scale=1.6, compact=True)
    c0.close()
    order = np.random.default_rng(5).integers(0, 20, (steps, B))
    data = [(img[idx], (o[idx], d[idx], t[idx])) for idx in (torch.as_tensor(r, device="cuda") for r in order)]
    rays = (o[20:22], d[20:22], t[20:22])
    u = torch.rand((B, wh, wh, 128), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))

    def run(n_steps, cb):
        nerf = NeRF(seed=0)
        nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=B, image_height=wh, image_width=wh, ray_chunks=1024,
                     white_background=True, deterministic=True)
        nerf.fit(data[:n_steps], epochs=1, callbacks=[cb] if cb else None, verbose=0)
        return nerf

    ref = run(warm, None)
    upd = OccupancyGridUpdater(update_every=16, warmup_steps=warm, resolution=64)
    a = run(warm, upd)
    assert upd.updates == 1 and a._ctx.get_option("occupancy_train") == 1
    for n in (0, 1):
        assert np.array_equal(a._ctx.get_weights(n), ref._ctx.get_weights(n))     # the dense steps before the warm-up are untouched
    upd = OccupancyGridUpdater(update_every=16, warmup_steps=warm, resolution=64)
    dense, occ = run(steps, None), run(steps, upd)
    assert upd.updates == 1 + (steps - warm) // 16
    st = occ.occupancy_train_stats()
    live = {k: v[0] / v[1] for k, v in st.items()}
    assert occ._ctx.get_option("occupancy_train") == 1 and live["coarse"] < 1 and live["fine"] < 1, live
    target = img[20:22]
    ps = {}
    for name, m in (("dense", dense), ("occ", occ)):
        f = m.predict_and_render_images(rays, u=u)[1]["image"]
        ps[name] = -10 * np.log10(max(float(((f - target) ** 2).mean()), 1e-20))
    rs = occ.occupancy_stats()
    log_stats("fit_grid_updater_compact_32x32", psnr_dense=ps["dense"], psnr_occ=ps["occ"], live_coarse=live["coarse"],
              live_fine=live["fine"], render_live_fine=rs["fine"][0] / max(rs["fine"][1], 1))
    assert rs["fine"][1] > 0                 # the grids stay attached after fit: the render ran behind them
    # measured on MI355X: 27.06 dB dense, 26.69 dB with the updater (live coarse 0.77 / fine 0.85 of the training samples)
    assert ps["occ"] >= ps["dense"] - 1.5, ps


def test_decay_max_kernel_equals_the_numpy_mirror():
    from keras_nerf_amd.runtime import occupancy_decay_max, occupancy_decay_max_reference
    g = torch.Generator(device="cuda").manual_seed(3)
    state = torch.rand((1000003,), device="cuda", generator=g) * 4
    sigma = torch.relu(torch.randn((1000003,), device="cuda", generator=g))
    for decay in (0.95, 0.0, 1.0, 0.5):
        ref = occupancy_decay_max_reference(state.cpu().numpy(), sigma.cpu().numpy(), decay)
        occupancy_decay_max(state, sigma, decay)
        assert np.array_equal(state.cpu().numpy(), ref), decay
