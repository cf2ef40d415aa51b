"""Training baked fields on RGBA, the parts that need no GPU: the NumPy reference (tests/baked_rgba_reference.py) against float64 torch
autograd of the O(S^2) definition and against central differences of its own loss, the recomposition identity, the keywords' parsing
and refusals, the routing of the launches, the host composition of render(background=), the two new symbols and the host-side refusals
of the two _rgba entry points.

Autograd bound: 1e-10 of the largest entry of the tensor (the rule of tests/test_baked_objective_host.py: both sides are float64
evaluations of the same function in different summation orders).  Central differences: h = 1e-5 and 1e-6 of the largest entry, as
tests/test_baked_train_host.py states them; the preconditions keep every clamp and kink 1e-3 away."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import baked_objective_reference as Q
from tests import baked_rgba_reference as P
from tests import baked_train_reference as T
from tests.test_baked_objective_host import _Recorder, _samples


def _torch_ray_loss(s, raw, index, delta, target, b, alpha, stored, kept, norm, kind, hd, lam_d, lam_e, lam_o):
    """the definition in torch, float64: the photograph over b, O(S^2) distortion, the clamped entropy, (O - alpha)^2"""
    s, raw = s[:kept], raw[:kept]
    a = 1 - torch.exp(-(s * delta))
    Tn = torch.cumprod(1 - a, 0)
    Tb = torch.cat([torch.ones(1, dtype=torch.float64), Tn[:-1]])
    w = Tb * a
    col = raw.clamp(0, 1)
    O = w.sum()
    b = torch.as_tensor(np.asarray(b, dtype=np.float64))
    pre = (w[:, None] * col).sum(0) + b * (1 - O)
    tgt = torch.as_tensor(np.asarray(target, dtype=np.float64))
    if alpha is not None:
        tgt = tgt + (1 - alpha) * (b - stored)
    d = pre.clamp(0, 1) - tgt
    ad = d.abs()
    if kind == Q.MSE:
        r = d * d
    elif kind == Q.MAE:
        r = ad
    elif kind == Q.HUBER:
        r = torch.where(ad <= hd, 0.5 * d * d, hd * (ad - 0.5 * hd))
    else:
        r = ad + torch.log1p(torch.exp(-2 * ad)) - np.log(2.0)
    m = torch.as_tensor((index[:kept] - index[0]).astype(np.float64) * delta)
    D = (w[:, None] * w[None, :] * (m[:, None] - m[None, :]).abs()).sum() + delta / 3.0 * (w * w).sum()
    ac = O.clamp(Q.CLAMP, 1 - Q.CLAMP)
    H = -ac * torch.log(ac) - (1 - ac) * torch.log(1 - ac)
    op = (O - (1.0 if alpha is None else alpha)) ** 2
    return r.sum() / (3.0 * norm) + lam_d * D / norm + lam_e * H / norm + lam_o * op / norm


# (fetched samples, density scale, gaps, termination, alpha, stored): thin .. opaque, exact 0 / 1 and interior alphas, no alpha at all
RAY_CASES = [(1, 8.0, False, 0.0, 0.0, 0.0), (2, 8.0, True, 0.0, 1.0, 1.0), (33, 1.0, True, 0.0, 0.35, 1.0), (33, 1.0, False, 0.0, None, 0.0),
             (33, 6.0, True, 0.05, 0.8, 0.0), (33, 1e-5, True, 0.0, 0.0, 1.0), (33, 12.0, True, 0.0, 0.6, 0.0)]
KIND_CASES = [(Q.MSE, 0.0), (Q.MAE, 0.0), (Q.HUBER, 0.2), (Q.LOG_COSH, 0.0)]


@pytest.mark.parametrize("kind,hd", KIND_CASES)
@pytest.mark.parametrize("n,density,gaps,termination,alpha,stored", RAY_CASES)
def test_ray_gradient_matches_autograd_of_the_definition(n, density, gaps, termination, alpha, stored, kind, hd):
    delta, norm, lam_d, lam_e, lam_o = 0.05, 7.0, 0.3, 0.02, 0.0 if alpha is None else 0.4
    s, raw, index = _samples(n, 13 * n + int(stored), density, gaps)
    target, b = np.array([0.2, 0.55, 0.9]), np.array([0.9, 0.05, 0.4])
    ref = P.ray_objective(s, raw, index, delta, target, b, alpha, stored, termination, norm, kind, hd, lam_d, lam_e, lam_o)
    kept = ref["kept"]
    if termination:
        assert 1 < kept < n, "the case is there for a cut"
    ts, traw = torch.tensor(s, requires_grad=True), torch.tensor(raw, requires_grad=True)
    L = _torch_ray_loss(ts, traw, index, delta, target, b, alpha, stored, kept, norm, kind, hd, lam_d, lam_e, lam_o)
    L.backward()
    gs, graw = ts.grad.numpy()[:kept], traw.grad.numpy()[:kept]
    value = ref["rho"] / (3 * norm) + lam_d * ref["D"] / norm + lam_e * ref["H"] / norm + lam_o * ref["op"] / norm
    assert abs(value - float(L.detach())) <= 1e-14
    assert np.abs(gs).max() > 0
    assert np.abs(ref["ds"] - gs).max() <= 1e-10 * np.abs(gs).max(), (np.abs(ref["ds"] - gs).max(), np.abs(gs).max())
    assert np.abs(ref["draw"] - graw).max() <= 1e-10 * max(np.abs(graw).max(), 1e-300)
    # the float32 form and the kernel's summation order are the same function
    for mirror in (False, True):
        r32 = P.ray_objective(s, raw, index, delta, target, b, alpha, stored, termination, norm, kind, hd, lam_d, lam_e, lam_o,
                              f=np.float32, mirror=mirror)
        assert r32["kept"] == kept and np.abs(r32["ds"] - ref["ds"]).max() <= 1e-4 * np.abs(ref["ds"]).max()
    # without background, alpha and weight it is the extended objective
    if alpha is None:
        for white in (0.0, 1.0):
            q = Q.ray_objective(s, raw, index, delta, target, white, termination, norm, kind, hd, lam_d, lam_e)
            p = P.ray_objective(s, raw, index, delta, target, np.full(3, white), None, stored, termination, norm, kind, hd, lam_d, lam_e)
            assert np.array_equal(q["ds"], p["ds"]) and np.array_equal(q["draw"], p["draw"]) and q["rho"] == p["rho"]


def test_opacity_term_reaches_a_ray_whose_differences_are_zero():
    s, raw, index = _samples(20, 4, 1.0, True)
    b = np.array([0.3, 0.6, 0.1])
    probe = P.ray_objective(s, raw, index, 0.05, np.zeros(3), b, None, 0.0, 0.0, 5.0)
    ref = P.ray_objective(s, raw, index, 0.05, probe["out"], b, None, 0.0, 0.0, 5.0, opacity=0.0)
    assert (ref["draw"] == 0).all() and (ref["ds"] == 0).all()
    ref = P.ray_objective(s, raw, index, 0.05, probe["out"], b, 1.0, 0.0, 0.0, 5.0, opacity=0.5)
    assert (ref["draw"] == 0).all() and (ref["ds"] < 0).all()             # alpha = 1 > O: more density everywhere lowers the loss
    empty = P.ray_objective(np.zeros(0), np.zeros((0, 3)), np.zeros(0, np.int64), 0.05, np.zeros(3), b, 0.25, 0.0, 0.0, 5.0, opacity=0.5)
    assert empty["kept"] == 0 and empty["op"] == 0.0625 and empty["ds"].size == 0


RES = (4, 4, 3)
LO, HI = (-1.0, -1.0, -0.6), (1.0, 1.0, 0.6)
STEP = 0.07
FD_H = 1e-5


@pytest.mark.parametrize("degree,termination,dense,kind,hd,stored", [(0, 0.0, 1.0, Q.MSE, 0.0, 0.0), (2, 0.0, 1.0, Q.HUBER, 0.3, 1.0),
                                                                     (2, 0.05, 3.0, Q.LOG_COSH, 0.0, 0.0), (0, 0.05, 3.0, Q.MAE, 0.0, 1.0)])
def test_lattice_gradient_matches_central_differences(degree, termination, dense, kind, hd, stored):
    from tests.test_baked_train_host import _case
    sigma, co, o, d, near, far, target = _case(degree, dense=dense)
    n = o.shape[0]
    rng = np.random.default_rng(17)
    bg = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    alpha = rng.uniform(0.05, 0.95, n).astype(np.float32)
    alpha[::3], alpha[1::5] = 0.0, 1.0
    support = T.support_cells(sigma)
    kw = dict(background=bg, alpha=alpha, stored=stored, termination=termination, loss_kind=kind, huber_delta=hd, distortion=0.5,
              opacity_entropy=0.05, opacity=0.3)
    args = (LO, HI, o, d, near, far, STEP, target, support)
    s64, co64 = sigma.astype(np.float64), co.astype(np.float64)
    info = {}
    L, terms, gs, gc = P.loss_and_grad(s64, co64, *args, **kw, info=info)
    assert abs(L - (terms["photometric"] + 0.5 * terms["distortion"] + 0.05 * terms["opacity_entropy"] + 0.3 * terms["opacity"])) <= 1e-15
    assert np.allclose(info["tgt"], P.recompose(target, alpha, bg, stored), rtol=0, atol=1e-16)
    raw, pre, Tn, opa = info["raw"], info["pre"], info["T"], info["opacity"]
    assert np.abs(raw).min() > 1e-3 and np.abs(raw - 1).min() > 1e-3 and np.abs(pre).min() > 1e-3 and np.abs(pre - 1).min() > 1e-3
    diff = np.clip(pre, 0, 1) - info["tgt"]
    assert (kind != Q.MAE or np.abs(diff).min() > 1e-3) and (kind != Q.HUBER or np.abs(np.abs(diff) - hd).min() > 1e-3)   # rho's kinks
    assert min(np.abs(opa - Q.CLAMP).min(), np.abs(opa - (1 - Q.CLAMP)).min()) > 1e-5
    if termination:
        assert (Tn < termination).sum() >= 3 and np.abs(Tn / termination - 1).min() > 1e-2
    # with the flag's colour, no alpha and weight 0 it is the extended objective's reference, bit for bit
    for white in (False, True):
        q = Q.loss_and_grad(s64, co64, *args, white, termination, kind, hd, 0.5, 0.05)
        p = P.loss_and_grad(s64, co64, *args, white_background=white, termination=termination, loss_kind=kind, huber_delta=hd,
                            distortion=0.5, opacity_entropy=0.05)
        assert q[0] == p[0] and np.array_equal(q[2], p[2]) and np.array_equal(q[3], p[3])
    worst = {"sigma": 0.0, "coef": 0.0}
    loss = lambda s, c: P.loss_and_grad(s, c, *args, **kw)[0]
    for p in rng.choice(s64.size, 24, replace=False):
        i = np.unravel_index(p, RES)
        a, b = s64.copy(), s64.copy()
        a[i] += FD_H; b[i] -= FD_H
        worst["sigma"] = max(worst["sigma"], abs((loss(a, co64) - loss(b, co64)) / (2 * FD_H) - gs[i]))
    for p in rng.choice(co64.size, 16, replace=False):
        i = np.unravel_index(p, co64.shape)
        a, b = co64.copy(), co64.copy()
        a[i] += FD_H; b[i] -= FD_H
        worst["coef"] = max(worst["coef"], abs((loss(s64, a) - loss(s64, b)) / (2 * FD_H) - gc[i]))
    print(f"degree {degree} kind {kind}: max |fd - analytic| / max |g| = {worst['sigma'] / np.abs(gs).max():.2e} (sigma), "
          f"{worst['coef'] / np.abs(gc).max():.2e} (coefficients)")
    assert worst["sigma"] <= 1e-6 * np.abs(gs).max() and worst["coef"] <= 1e-6 * np.abs(gc).max()


@pytest.mark.parametrize("stored", [0.0, 1.0])
def test_recomposition_identity(stored):
    """the loader stores alpha rgb + (1 - alpha) B0; target + (1 - alpha)(b - B0) is the photograph over b"""
    rng = np.random.default_rng(3)
    rgb, b = rng.uniform(0, 1, (200, 3)), rng.uniform(0, 1, (200, 3))
    alpha = rng.uniform(0, 1, 200)
    alpha[:20], alpha[20:40] = 0.0, 1.0
    stored_target = alpha[:, None] * rgb + (1 - alpha[:, None]) * stored
    want = alpha[:, None] * rgb + (1 - alpha[:, None]) * b
    got = P.recompose(stored_target, alpha, b, stored)
    assert np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps
    assert np.array_equal(got[20:40], stored_target[20:40])               # alpha = 1: the target as it is
    assert np.abs(got[:20] - b[:20]).max() <= 2 * np.finfo(np.float64).eps    # alpha = 0: the background itself


def test_keywords_are_parsed_and_refused():
    from keras_nerf_amd.baked_train import RgbaTargets
    r = RgbaTargets()
    assert (r.white, r.mode, r.opacity, r.stored, r.seed) == (False, None, 0.0, 0.0, 0)
    assert RgbaTargets(True).white and RgbaTargets(True).stored == 1.0
    assert RgbaTargets(False, "white").white and RgbaTargets(True, "white").white and RgbaTargets(False, "white").stored == 1.0
    assert not RgbaTargets(False, "black").white and RgbaTargets(False, "black").mode is None
    assert RgbaTargets(False, "random", 1e-3, "white", 7).__dict__.items() >= dict(mode="random", opacity=1e-3, stored=1.0, seed=7).items()
    assert RgbaTargets(False, (0.25, 0.5, 1)).colour == (0.25, 0.5, 1.0) and RgbaTargets(True, None, 0.0, "black").stored == 0.0
    for kw in (dict(white_background=True, background="black"), dict(white_background=True, background="random"),
               dict(white_background=True, background=(1, 1, 1)), dict(background="grey"), dict(background=(0.1, 0.2)),
               dict(background=(0.1, 0.2, 1.5)), dict(background=(0.1, float("nan"), 0.5)), dict(background=0.5),
               dict(opacity_loss=-1e-3), dict(opacity_loss=float("inf")), dict(opacity_loss=float("nan")), dict(opacity_loss="1"),
               dict(opacity_loss=True), dict(target_background="grey"), dict(target_background=1), dict(background_seed=1.5),
               dict(background_seed=None)):
        with pytest.raises(ValueError):
            RgbaTargets(**kw)


def test_a_launch_record_is_made_or_refused():
    from keras_nerf_amd.baked_train import RgbaTargets
    cpu = torch.device("cpu")
    tg3, tg4 = torch.zeros((6, 3)), torch.rand((6, 4))
    assert RgbaTargets().record(None, 6, cpu) is None and RgbaTargets(True, "white").record(None, 6, cpu) is None
    rgb, alpha = RgbaTargets().split_target(tg4, 6)
    assert torch.equal(rgb, tg4[:, :3]) and torch.equal(alpha, tg4[:, 3]) and rgb.is_contiguous() and alpha.is_contiguous()
    assert RgbaTargets().split_target(tg3, 6)[1] is None
    for bad in (tg3[:5], tg3[:, :2], torch.zeros((6, 5)), torch.zeros(18)):
        with pytest.raises(ValueError, match="target"):
            RgbaTargets().split_target(bad, 6)
    # an [n,4] target alone is an rgba launch: the alpha recomposes the target
    rec = RgbaTargets(True, None, 0.0, "black").record(alpha, 6, cpu)
    assert rec.background is None and rec.alpha == alpha.data_ptr() and rec.stored_background == 0.0 and rec.opacity == 0.0
    r = RgbaTargets(False, "random", 0.25, None, 5)
    a, b = r.record(alpha, 6, cpu), r.record(alpha, 6, cpu)
    first, second = a._keep[0], r.last_background
    gen = torch.Generator().manual_seed(5)
    assert torch.equal(first, torch.rand((6, 3), generator=gen)) and torch.equal(second, torch.rand((6, 3), generator=gen))
    assert a.background == first.data_ptr() and b.background == second.data_ptr() and a.opacity == 0.25
    colour = RgbaTargets(False, (0.25, 0.5, 1.0))
    rec = colour.record(None, 6, cpu)
    assert torch.equal(colour.last_background, torch.tensor([[0.25, 0.5, 1.0]]).expand(6, 3)) and rec.alpha is None
    over = torch.rand((6, 3))
    rec = colour.record(None, 6, cpu, background=over)                     # a per-call tensor overrides the keyword
    assert torch.equal(colour.last_background, over) and rec.background == colour.last_background.data_ptr()
    for kw, al in ((dict(background="random"), None), (dict(opacity_loss=0.1), None)):
        with pytest.raises(ValueError, match=r"\[n, 4\]"):
            RgbaTargets(**kw).record(al, 6, cpu)
    for bad in (torch.rand((5, 3)), torch.rand((6, 4)), torch.full((6, 3), 1.5), torch.full((6, 3), -0.1), torch.full((6, 3), float("nan")),
                np.full((6, 3), np.inf)):
        with pytest.raises(ValueError, match="background"):
            RgbaTargets().record(None, 6, cpu, background=bad)


def _bare(cls, objective, **rgba):
    from keras_nerf_amd.baked_train import RgbaTargets
    opt = object.__new__(cls)
    opt.field = types.SimpleNamespace(device=torch.device("cpu"), cell_size=(0.1, 0.1, 0.1))
    opt._rgba = RgbaTargets(**rgba)
    opt.step, opt.white_background, opt.termination, opt.lanes_per_ray = 0.05, opt._rgba.white, 0.0, 0
    opt.objective, opt._terms, opt._c = objective, None, C.c_int(0)
    return opt


def test_the_new_keywords_route_to_the_rgba_entry_points_and_nothing_else_moves(monkeypatch):
    from keras_nerf_amd import _lib, baked_bricks_grow, baked_bricks_train, baked_train
    from keras_nerf_amd.baked_train import check_objective
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(baked_train, "_stream", lambda dev: None)
    monkeypatch.setattr(baked_bricks_train, "_stream", lambda dev: None)
    o, d = np.zeros((5, 3), np.float32), np.ones((5, 3), np.float32)
    tg3, tg4 = np.zeros((5, 3), np.float32), np.full((5, 4), 0.5, np.float32)
    for cls, name in ((baked_train.BakedFieldOptimizer, "knerf_baked_train_rays"),
                      (baked_bricks_train.BrickFieldOptimizer, "knerf_baked_bricks_train_rays"),
                      (baked_bricks_grow.BrickGridTrainer, "knerf_baked_bricks_train_rays")):
        for objective, suffix in ((None, ""), (check_objective("huber", None), "_ext")):
            for kw in (dict(), dict(background="black"), dict(background="white"), dict(white_background=True, background="white"),
                       dict(target_background="white"), dict(background_seed=3)):
                rec.calls.clear()
                opt = _bare(cls, objective, **kw)
                opt.accumulate(o, d, 0.0, 1.0, tg3)
                assert rec.calls == [name + suffix] and opt.last_background is None, (cls.__name__, kw, rec.calls)
                assert opt.white_background == (kw.get("background") == "white")
            for kw, tg, extra in ((dict(background="random"), tg4, {}), (dict(opacity_loss=0.1), tg4, {}), (dict(), tg4, {}),
                                  (dict(background=(0.5, 0.5, 0.5)), tg3, {}), (dict(), tg3, dict(background=np.full((5, 3), 0.25)))):
                rec.calls.clear()
                opt = _bare(cls, objective, **kw)
                loss = opt.accumulate(o, d, 0.0, 1.0, tg, **extra)
                assert rec.calls == [name + "_rgba"], (cls.__name__, kw, rec.calls)
                terms = opt.objective_terms()
                assert loss.dtype == torch.float64 and tuple(terms) == P.TERMS
                assert (opt.last_background is None) == (not kw.get("background") and not extra)
            for kw in (dict(background="random"), dict(opacity_loss=0.1)):
                rec.calls.clear()
                with pytest.raises(ValueError):
                    _bare(cls, objective, **kw).accumulate(o, d, 0.0, 1.0, tg3)
                assert rec.calls == []


def test_constructors_take_the_keywords():
    import inspect
    from keras_nerf_amd import baked, baked_bricks_grow, baked_bricks_train, baked_quant, baked_train
    from keras_nerf_amd.data import loader, raybatch
    for fn in (baked.BakedField.optimizer, baked_train.BakedFieldOptimizer.__init__, baked_train.brick_optimizer,
               baked_bricks_train.BrickFieldOptimizer.__init__, baked_bricks_grow.BrickGridTrainer.__init__, baked_bricks_grow.grid_trainer):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("background", "opacity_loss", "target_background", "background_seed")] == [None, 0.0, None, 0], fn
    for cls in (baked_train.BakedFieldOptimizer, baked_bricks_train.BrickFieldOptimizer):
        p = inspect.signature(cls.accumulate).parameters
        assert p["background"].default is None and p["n_total"].default is None
    for cls in (baked.BakedField, baked.BrickBakedField, baked_quant.QuantizedBrickField):
        assert inspect.signature(cls.render).parameters["background"].default is None
    assert inspect.signature(loader.RayImageDataset.ray_batches).parameters["alpha"].default is False
    assert inspect.signature(raybatch.RayBatchDataset.__init__).parameters["alpha"].default is False
    with pytest.raises(ValueError, match="QuantizedBrickField"):
        baked_train.brick_optimizer(object.__new__(baked_quant.QuantizedBrickField), 0.1, 0.1, background="random")


def test_render_background_composition():
    from keras_nerf_amd.baked import compose_background, render_over
    rng = np.random.default_rng(8)
    opacity = rng.uniform(0, 1, 50).astype(np.float32)
    opacity[:5], opacity[5:10] = 0.0, 1.0
    image = (opacity[:, None] * rng.uniform(0, 1, (50, 3))).astype(np.float32)
    bg = rng.uniform(0, 1, (50, 3)).astype(np.float32)
    want = np.clip(image + (np.float32(1) - opacity)[:, None] * bg, 0, 1)
    assert np.array_equal(compose_background(image, opacity, bg), want) and want.dtype == np.float32
    assert np.array_equal(compose_background(image, opacity, bg)[:5], bg[:5]) and np.array_equal(want[5:10], image[5:10])
    assert np.array_equal(compose_background(image, opacity, np.zeros(3, np.float32)), image)
    got = compose_background(torch.as_tensor(image), torch.as_tensor(opacity), torch.as_tensor(bg))
    assert np.array_equal(got.numpy(), want)
    assert float(compose_background(torch.full((1, 3), 0.9), torch.tensor([0.5]), torch.ones(3)).max()) == 1.0      # clipped

    class Field:
        device = torch.device("cpu")

        def render(self, *args, white_background, outputs, **kw):
            self.seen = (args, white_background, tuple(outputs), kw)
            full = {"image": torch.as_tensor(image), "depth": torch.zeros(50), "opacity": torch.as_tensor(opacity)}
            return {k: full[k] for k in outputs}

    f = Field()
    out = render_over(f, (0.2, 0.4, 0.6), False, ("image", "depth"), (1, 2, 3, 4), dict(step=0.1))
    assert sorted(out) == ["depth", "image"] and f.seen == ((1, 2, 3, 4), False, ("image", "depth", "opacity"), dict(step=0.1))
    assert np.array_equal(out["image"].numpy(), np.clip(image + (np.float32(1) - opacity)[:, None] * np.array([0.2, 0.4, 0.6], np.float32), 0, 1))
    assert np.array_equal(render_over(f, bg, False, "image", (), {})["image"].numpy(), want)
    assert sorted(render_over(f, bg, False, ("depth",), (), {})) == ["depth"] and f.seen[2] == ("depth",)
    for bad, white in (((1, 1, 1), True), ((1, 1), False), ((0.5, 0.5, 2.0), False), ("white", False), (bg[:10], False),
                       (np.full((50, 3), 1.5, np.float32), False), (torch.full((50, 3), float("nan")), False)):
        with pytest.raises(ValueError):
            render_over(f, bad, white, ("image",), (), {})


def test_the_new_symbols_are_declared_and_bound():
    import os
    import re
    from keras_nerf_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "knerf.h")).read()
    for name, ext in (("knerf_baked_train_rays_rgba", "knerf_baked_train_rays_ext"),
                      ("knerf_baked_bricks_train_rays_rgba", "knerf_baked_bricks_train_rays_ext")):
        assert re.search(r"\bint " + name + r"\(", header), name
        res, args = _lib.SIGNATURES[name]
        eres, eargs = _lib.SIGNATURES[ext]
        assert res is eres and args[:-1] == eargs and args[-1] is C.POINTER(_lib.KnerfBakedRgba)
    assert re.search(r"typedef struct knerf_baked_rgba \{[^}]*background;[^}]*alpha;[^}]*stored_background;[^}]*opacity;[^}]*\} knerf_baked_rgba;",
                     header)
    assert [f[0] for f in _lib.KnerfBakedRgba._fields_] == ["background", "alpha", "stored_background", "opacity"]
    assert C.sizeof(_lib.KnerfBakedRgba) == 24


def test_rgba_entry_points_refuse_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID decided on the host, no device needed: everything _ext refuses and the record's own errors"""
    from keras_nerf_amd import _lib
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    p = C.c_void_p(4096)                                                  # never dereferenced: every call below is refused first

    def dense(degree=2, records=p, grad=p, n_slots=10):
        f = _lib.KnerfBakedField(records, p, (C.c_int32 * 3)(9, 7, 6), degree, (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1))
        return _lib.KnerfBakedTrain(f, p, grad, n_slots)

    def bricks(degree=2, records=p, grad=p, n_bricks=3, log2=2):
        f = _lib.KnerfBakedBricks(records, p, p, (C.c_int32 * 3)(9, 7, 6), degree, (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1),
                                  log2, n_bricks)
        return _lib.KnerfBakedBricksTrain(f, grad)

    def rgba(background=p, alpha=p, stored=0.0, opacity=0.1):
        return _lib.KnerfBakedRgba(background, alpha, stored, opacity)

    huber = _lib.KnerfObjective(_lib.LOSS_HUBER, 0.1, 0.01, 1e-3, 3)
    for fn, state in ((lib.knerf_baked_train_rays_rgba, dense), (lib.knerf_baked_bricks_train_rays_rgba, bricks)):
        def call(st, ob, rg, o=p, target=p, n=10, n_norm=0, step=0.05, term=0.0, flags=0, terms=p):
            return fn(None, C.byref(st) if st is not None else None, o, p, None, None, 0.0, 1.0, target, n, n_norm, step, term, flags, None,
                      C.byref(ob) if ob is not None else None, terms, C.byref(rg) if rg is not None else None)
        for ob in (None, huber):
            for rg in (None, rgba(), rgba(None, None, 1.0, 0.0), rgba(None, p, 1.0, 0.0), rgba(p, None, 0.0, 0.0)):
                assert call(state(), ob, rg, n=0) == 0                     # no rays: nothing to launch
                assert call(None, ob, rg) == INV
                for bad in (dict(records=None), dict(grad=None), dict(degree=4)):
                    assert call(state(**bad), ob, rg) == INV, bad
                for bad in (dict(o=None), dict(target=None), dict(step=0.0), dict(term=1.0), dict(flags=4), dict(flags=2 << 8),
                            dict(n=1 << 36), dict(n_norm=1 << 36)):
                    assert call(state(), ob, rg, **bad) == INV, bad
            for bad in (dict(stored=0.5), dict(stored=-1.0), dict(stored=2.0), dict(stored=float("nan")), dict(opacity=-0.1),
                        dict(opacity=float("nan")), dict(opacity=float("inf")), dict(alpha=None), dict(alpha=None, background=None),
                        dict(background=None, alpha=None, opacity=0.0, stored=0.5)):
                assert call(state(), ob, rgba(**bad)) == INV, bad
                assert call(state(), ob, rgba(**bad), n=0) == INV, bad
        for bad in ((4, 0.1, 0.0, 0.0), (_lib.LOSS_HUBER, 0.0, 0.0, 0.0), (_lib.LOSS_MSE, 0.0, -1.0, 0.0), (_lib.LOSS_MAE, 0.0, 0.0, float("nan"))):
            assert call(state(), _lib.KnerfObjective(*bad, 3), rgba()) == INV, bad
