"""Early ray termination of the render passes (options termination_threshold / termination_segment, csrc/termination.hip) on the GPU:
eps = 0 changes no bit; the cut rule on the coarse and the fine pass against dense references (per-ray transmittance in fp64 from the
dense weights: bits before the first boundary with T < eps, exactly 0 behind it); the image and depth bounds on black and white
backgrounds; behind an occupancy grid the evaluated set is "occupied and not cut"; the general-shape and padded paths follow the same
rule; merged launches, training, forward_chunk and the queries are unaffected; a trained scene renders close to dense."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import occupancy_reference as OM
from tests import termination_reference as M
from tests.test_gpu_forward import log_stats

pytestmark = pytest.mark.gpu
LO, HI = (-1.5,) * 3, (1.5,) * 3
EPS, L = 1e-3, 16


def _ctx(P, white=True, **kw):
    from keras_nerf_amd.runtime import KnerfContext
    ctx = KnerfContext(white_background=white, n_layers=P["cfg"].n_layers, dense_units=P["cfg"].dense_units,
                       skip_layer=P["cfg"].skip_layer, pos_emb_xyz=P["cfg"].pos_emb_xyz, pos_emb_dir=P["cfg"].pos_emb_dir, **kw)
    ctx.set_weights(0, O.flatten_params(P["cp"])); ctx.set_weights(1, O.flatten_params(P["fp"]))
    return ctx


def _rays(P):
    N = P["N"]
    return tuple(P[k].reshape(N, -1).astype(np.float32) for k in ("o", "d", "t", "u"))


def _render(ctx, P, ray_chunks=128):
    o, d, t, u = _rays(P)
    N, Nc = P["N"], ctx.n_coarse
    Na = Nc + ctx.n_fine
    e = lambda *s: torch.full(s, float("nan"), device="cuda")
    out = dict(c_image=e(N, 3), c_depth=e(N), c_weights=e(N, Nc), f_image=e(N, 3), f_depth=e(N), f_weights=e(N, Na), t_fine=e(N, Na))
    ctx.render_batch(o, d, t, u, seed=5, ray_chunks=ray_chunks, out=out)
    torch.cuda.synchronize()
    return out


def _same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


def _problem(**kw):
    from tests.problem import make_problem
    return make_problem(n_images=kw.pop("n_images", 1), wh=16, weight_scale=kw.pop("weight_scale", 2.0), bias_std=0.05, **kw)


def _check_cut(w_ref, w_term, eps=EPS, seg=L):
    """the cut rule of one pass: w_ref = the weights without termination (dense, or grid-only), w_term = the terminated render's.
    Returns (lo, hi) int [R]: the cut of each ray (lo == hi) or, for a ray whose T at some boundary lies within a relative 1e-3 of
    eps, the range its cut may lie in."""
    wr, wt = w_ref.cpu().numpy(), w_term.cpu().numpy()
    R, S = wr.shape
    cs, T = M.boundary_transmittance(wr, seg)
    first = lambda m: np.where(m.any(axis=1), cs[np.argmax(m, axis=1)] if len(cs) else S, S)
    lo, hi = first(T < eps * (1 + 1e-3)), first(T < eps * (1 - 1e-3))
    idx = np.arange(S)[None, :]
    before, behind = idx < lo[:, None], idx >= hi[:, None]
    assert np.array_equal(wt[before].view(np.uint32), wr[before].view(np.uint32)), "weights in front of the cut differ"
    assert (wt[behind] == 0).all(), "terminated samples have non-zero weights"
    return lo, hi


def _check_bounds(ref, term, t_max=6.0, eps=EPS):
    for k in ("image", "depth"):
        tol = eps + 1e-6 if k == "image" else eps * t_max + 1e-5
        diff = float((ref[k] - term[k]).abs().max())
        assert diff <= tol, (k, diff, tol)


def _terminated(ctx, P, eps=EPS, seg=L, **kw):
    ctx.set_option("termination_segment", seg)
    ctx.set_option("termination_threshold", eps)
    ctx.termination_stats(reset=True)
    out = _render(ctx, P, **kw)
    return out, ctx.termination_stats()


def _check_pass_pair(ctx, P, dense, term, stats, min_frac=0.0):
    """coarse against the dense render, fine against forward_chunk(FINE) on the terminated render's t_fine; stats within the cuts"""
    from keras_nerf_amd.runtime import FINE
    o, d, _, _ = _rays(P)
    N, Nc = P["N"], ctx.n_coarse
    Na = Nc + ctx.n_fine
    lo, hi = _check_cut(dense["c_weights"], term["c_weights"])
    frac = 1 - lo.sum() / (N * Nc)
    assert frac >= min_frac, frac
    _check_bounds({"image": dense["c_image"], "depth": dense["c_depth"]}, {"image": term["c_image"], "depth": term["c_depth"]})
    fi, fd, fw = ctx.forward_chunk(FINE, o, d, term["t_fine"])
    torch.cuda.synchronize()
    lo_f, hi_f = _check_cut(fw, term["f_weights"])
    _check_bounds({"image": fi, "depth": fd}, {"image": term["f_image"], "depth": term["f_depth"]})
    (lc, tc), (lf, tf) = stats
    assert tc == N * Nc and tf == N * Na
    assert lo.sum() <= lc <= hi.sum() and lo_f.sum() <= lf <= hi_f.sum(), (lc, lo.sum(), hi.sum(), lf, lo_f.sum(), hi_f.sum())
    exact = lo == hi
    log_stats("termination_cut", coarse_terminated=frac, fine_terminated=1 - lo_f.sum() / (N * Na), coarse_near=(~exact).sum(),
              fine_near=(lo_f != hi_f).sum())
    return frac


@pytest.mark.parametrize("merge", [None, 0])
def test_threshold_zero_changes_no_bit(merge):
    P = _problem()
    opts = None if merge is None else dict(merge_render_rays=merge)
    a, b = _ctx(P, options=opts), _ctx(P, options=opts)
    ref = _render(a, P)
    b.set_option("termination_threshold", 1e-2)
    on = _render(b, P)
    assert not torch.equal(on["f_image"], ref["f_image"])
    b.set_option("termination_threshold", 0)
    b.termination_stats(reset=True)
    _same(_render(b, P), ref)
    assert b.termination_stats() == ((0, 0), (0, 0))          # a pass with eps = 0 is not counted
    a.close(); b.close()


@pytest.mark.parametrize("white", [True, False])
def test_cut_rule_and_bounds_on_both_passes(white):
    P = _problem()
    ctx = _ctx(P, white=white)
    dense = _render(ctx, P)
    term, stats = _terminated(ctx, P)
    assert ctx.get_option("termination_threshold") == EPS and ctx.get_option("termination_segment") == L
    _check_pass_pair(ctx, P, dense, term, stats, min_frac=0.2)
    ctx.close()


def test_segment_lengths():
    """L = 1, a length that does not divide the sample counts, and one longer than the coarse pass"""
    P = _problem()
    ctx = _ctx(P)
    dense = _render(ctx, P)
    for seg in (1, 24, 100):
        term, stats = _terminated(ctx, P, seg=seg)
        lo, hi = _check_cut(dense["c_weights"], term["c_weights"], seg=seg)
        (lc, _), _ = stats
        assert lo.sum() <= lc <= hi.sum()
        if seg == 100:                                          # longer than the 64 coarse samples: nothing is cut there
            assert torch.equal(term["c_weights"], dense["c_weights"]) and lc == P["N"] * 64
    ctx.close()


def _grids(seed, cells=(16, 16, 16)):
    rng = np.random.default_rng(seed)
    return {0: rng.random(cells) < 0.5, 1: rng.random(cells[::-1]) < 0.5}


def test_grid_and_termination():
    """behind a grid: the evaluated set is exactly occupied and not cut, the rest is bit for bit the grid-only render"""
    from keras_nerf_amd.debug import debug_buffer
    from keras_nerf_amd.runtime import COARSE, FINE, _ptr
    P = _problem()
    o, d, t, u = _rays(P)
    N, Nc = P["N"], 64
    Na = 192
    ctx = _ctx(P)
    g = _grids(21)
    for net in (COARSE, FINE):
        ctx.set_occupancy(net, g[net], LO, HI, "occupied")
    ctx.occupancy_stats(reset=True)
    grid_only = ctx.render_chunk(o, d, t, u, seed=3)
    torch.cuda.synchronize()
    occ_ref = ctx.occupancy_stats()
    ctx.set_option("termination_segment", L)
    ctx.set_option("termination_threshold", EPS)
    ctx.termination_stats(reset=True)
    term = ctx.render_chunk(o, d, t, u, seed=3)
    torch.cuda.synchronize()
    raw = debug_buffer(ctx, 3).view(torch.float32)[:N * Na * 4].reshape(N, Na, 4).clone()
    (lc, tc), (lf, tf) = ctx.termination_stats()
    occ = ctx.occupancy_stats()                                  # the grid's verdict on every sample, as without termination
    assert occ[0] == occ_ref[0]
    # coarse: against the grid-only render
    live_c = OM.lookup(OM.ray_points(o, d, t), g[COARSE], LO, HI, "occupied")
    lo, hi = _check_cut(grid_only["c_weights"], term["c_weights"])
    idx = np.arange(Nc)[None, :]
    assert (live_c & (idx < lo[:, None])).sum() <= lc <= (live_c & (idx < hi[:, None])).sum() and tc == N * Nc
    assert (lo < Nc).mean() > 0.05
    # fine: the grid-only raw on the terminated render's t_fine (query + the mirror's verdict), composited
    tf_t = term["t_fine"]
    live_f = OM.lookup(OM.ray_points(o, d, tf_t.cpu().numpy()), g[FINE], LO, HI, "occupied")
    assert occ[1] == (int(live_f.sum()), N * Na)                 # (the fine samples moved with the coarse weights behind the cut)
    q = ctx.query_points(FINE, OM.ray_points(o, d, tf_t.cpu().numpy()).reshape(-1, 3), np.repeat(d, Na, 0)).reshape(N, Na, 4)
    q[torch.as_tensor(~live_f, device="cuda")] = 0.0
    w_ref, img = torch.empty((N, Na), device="cuda"), torch.empty((N, 3), device="cuda")
    assert ctx.lib.knerf_composite(ctx._stream(), _ptr(q), _ptr(tf_t.contiguous()), N, Na, 1, _ptr(img), None, _ptr(w_ref)) == 0
    torch.cuda.synchronize()
    lo_f, hi_f = _check_cut(w_ref, term["f_weights"])
    idx = np.arange(Na)[None, :]
    ev_lo, ev_hi = live_f & (idx < lo_f[:, None]), live_f & (idx < hi_f[:, None])
    exact = torch.as_tensor(lo_f == hi_f, device="cuda")           # the evaluated set of every ray whose cut is certain
    ev = torch.as_tensor(ev_lo, device="cuda")
    assert bool(exact.float().mean() > 0.95)
    assert torch.equal(raw[exact][ev[exact]], q[exact][ev[exact]]) and bool((raw[exact][~ev[exact]] == 0).all())
    assert ev_lo.sum() <= lf <= ev_hi.sum() and tf == N * Na
    assert (img - term["f_image"]).abs().max().item() <= EPS + 1e-6
    ctx.close()


@pytest.mark.parametrize("shape", ["force_generic", "padded_192"])
def test_other_shapes_follow_the_same_rule(shape):
    cfg = {"padded_192": O.NerfConfig(dense_units=192), "force_generic": O.NerfConfig()}[shape]
    P = _problem(cfg=cfg)
    ctx = _ctx(P, force_generic=shape == "force_generic")
    assert bool(ctx.get_option("general_shape_path")) == (shape == "force_generic")
    dense = _render(ctx, P)
    term, stats = _terminated(ctx, P)
    frac = _check_pass_pair(ctx, P, dense, term, stats)
    assert frac > 0.05, frac
    ctx.close()


def test_merged_launches_are_bit_identical():
    P = _problem()
    outs = []
    for merge in (65536, 0):
        ctx = _ctx(P, options=dict(merge_render_rays=merge))
        outs.append(_terminated(ctx, P, ray_chunks=64))
        ctx.close()
    _same(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1]


def test_training_forward_chunk_and_queries_never_terminate():
    from keras_nerf_amd.runtime import COARSE, FINE
    P = _problem(n_images=2)
    N = P["N"]
    o, d, t, u = _rays(P)
    img = P["img"].reshape(N, 3)
    pts = OM.ray_points(o[:64], d[:64], t[:64]).reshape(-1, 3)
    res = []
    for eps in (0.0, 1e-2):
        ctx = _ctx(P, options=dict(deterministic=1))
        ctx.set_option("termination_threshold", eps)
        fwd = [ctx.forward_chunk(n, o, d, t) for n in (COARSE, FINE)]
        q = ctx.query_points(FINE, pts, np.repeat(d[:64], 64, 0))
        qg = ctx.query_grid(COARSE, (9, 9, 9), LO, HI)[0]
        loss = torch.zeros(2, device="cuda")
        ci, fi = torch.empty((N, 3), device="cuda"), torch.empty((N, 3), device="cuda")
        ctx.train_batch(o, d, t, img, u, seed=1, ray_chunks=128, loss=loss, c_image=ci, f_image=fi)
        g = (ctx.grads(0), ctx.grads(1))
        ctx.apply_adam()
        torch.cuda.synchronize()
        res.append((loss.clone(), ci, fi, *g, *[x for f in fwd for x in f], q, qg))
        assert ctx.termination_stats() == ((0, 0), (0, 0))
        res[-1] += (torch.as_tensor(ctx.get_weights(0)), torch.as_tensor(ctx.get_weights(1)))
        ctx.close()
    for x, y in zip(*res):
        assert torch.equal(x, y)


def test_option_validation():
    P = _problem()
    ctx = _ctx(P)
    for name, bad in (("termination_threshold", -1e-3), ("termination_threshold", 1.0), ("termination_threshold", float("nan")),
                      ("termination_threshold", float("inf")), ("termination_segment", 0), ("termination_segment", 1025),
                      ("termination_segment", 2.5)):
        with pytest.raises(ValueError):
            ctx.set_option(name, bad)
    assert ctx.get_option("termination_threshold") == 0 and ctx.get_option("termination_segment") == 32
    ctx.close()


def test_trained_scene_renders_close_to_dense():
    """the compact procedural scene after 300 steps at 32 x 32: NeRF.set_ray_termination with its default threshold"""
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene
    wh, batch = 32, 2
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=wh, n_views=24, scale=1.6, compact=True)
    c0.close()
    nerf = NeRF(seed=0)
    nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=batch, image_height=wh, image_width=wh, ray_chunks=1024, white_background=True)
    order = np.random.default_rng(5).integers(0, 20, (300, batch))
    for s in range(300):
        idx = torch.as_tensor(order[s], device="cuda")
        nerf.train_step((img[idx], (o[idx], d[idx], t[idx])), with_metrics=False)
    nerf._ctx.poll_nonfinite(wait=True)
    rays = (o[20:22], d[20:22], t[20:22])
    u = torch.rand((batch, wh, wh, 128), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    dense = nerf.predict_and_render_images(rays, u=u)[1]["image"]
    # measured on MI355X over three training runs: PSNR 133.5 to 136.9 dB at the default (1e-4, L = 32); 75.9 to 79.0 dB with 98.4 %
    # of the fine samples evaluated at (1e-3, L = 16)
    for (eps, seg), floor in (((None, None), 100.0), ((1e-3, 16), 65.0)):
        if eps is None:
            nerf.set_ray_termination()
        else:
            nerf.set_ray_termination(eps, seg)
        nerf.termination_stats(reset=True)
        cut = nerf.predict_and_render_images(rays, u=u)[1]["image"]
        st = nerf.termination_stats()
        live = {k: v[0] / v[1] for k, v in st.items()}
        mse = float(((cut - dense) ** 2).mean())
        psnr = -10 * np.log10(max(mse, 1e-20))
        log_stats(f"trained_compact_32x32_step300_termination_{eps}_{seg}", psnr=psnr, evaluated_coarse=live["coarse"], evaluated_fine=live["fine"])
        assert psnr >= floor, (eps, psnr)
        if eps is not None:
            assert live["fine"] < 0.995, live
    nerf.set_ray_termination(0)
    assert torch.equal(nerf.predict_and_render_images(rays, u=u)[1]["image"], dense)
