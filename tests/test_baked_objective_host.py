"""The extended objective of the baked-field optimisers, the parts that need no GPU: the NumPy reference
(tests/baked_objective_reference.py) against float64 torch autograd of the O(S^2) definition and against central differences of its own
loss, the keywords' parsing and refusals on every constructor, the routing of the plain objective to the plain entry point, the two new
symbols, and the host-side refusals of the two _ext entry points.

Autograd bound: 1e-10 of the largest entry of the tensor (both sides are float64 evaluations of the same function in different
summation orders; the entries are sums of at most 33 x 33 products of order 1, so rounding stays near 1e-14 of the largest entry).
Central differences: step and tolerance as tests/test_baked_train_host.py states them (h = 1e-5, 1e-6 of the largest entry); the
preconditions here add the new kinks: no |d| within 1e-3 of huber_delta, no opacity within 1e-3 of an edge of the entropy clamp."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

from tests import baked_objective_reference as Q
from tests import baked_train_reference as T

KIND_CASES = [(Q.MSE, 0.0), (Q.MAE, 0.0), (Q.HUBER, 0.05), (Q.HUBER, 0.4), (Q.LOG_COSH, 0.0)]


def _torch_ray_loss(s, raw, index, delta, target, bg, kept, norm, kind, hd, lam_d, lam_e):
    """the definition in torch, float64: O(S^2) distortion, the entropy through torch.clamp, the cut held at `kept` samples"""
    s, raw = s[:kept], raw[:kept]
    alpha = 1 - torch.exp(-(s * delta))
    Tn = torch.cumprod(1 - alpha, 0)
    Tb = torch.cat([torch.ones(1, dtype=torch.float64), Tn[:-1]])
    w = Tb * alpha
    col = raw.clamp(0, 1)
    O = w.sum()
    pre = (w[:, None] * col).sum(0) + bg * (1 - O)
    d = pre.clamp(0, 1) - torch.as_tensor(np.asarray(target, dtype=np.float64))
    a = d.abs()
    if kind == Q.MSE:
        r = d * d
    elif kind == Q.MAE:
        r = a
    elif kind == Q.HUBER:
        r = torch.where(a <= hd, 0.5 * d * d, hd * (a - 0.5 * hd))
    else:
        r = a + torch.log1p(torch.exp(-2 * a)) - np.log(2.0)
    m = torch.as_tensor((index[:kept] - index[0]).astype(np.float64) * delta)
    D = (w[:, None] * w[None, :] * (m[:, None] - m[None, :]).abs()).sum() + delta / 3.0 * (w * w).sum()
    ac = O.clamp(Q.CLAMP, 1 - Q.CLAMP)
    H = -ac * torch.log(ac) - (1 - ac) * torch.log(1 - ac)
    return r.sum() / (3.0 * norm) + lam_d * D / norm + lam_e * H / norm, D, H


def _samples(n, seed, density, gaps):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.2, 1.0, n) * density
    raw = rng.uniform(-0.3, 1.3, (n, 3))
    raw[np.abs(raw) < 1e-3] = 0.5
    index = 5 + np.cumsum(rng.integers(1, 4 if gaps else 2, n))
    return s, raw, index.astype(np.int64)


# (fetched samples, density scale, gaps, white, termination): thin .. opaque, O below and above the entropy clamp, a terminated ray
RAY_CASES = [(1, 8.0, False, False, 0.0), (1, 8.0, False, True, 0.0), (2, 8.0, True, True, 0.0), (33, 1.0, True, False, 0.0),
             (33, 1.0, False, True, 0.0), (33, 6.0, True, True, 0.05), (33, 1e-5, True, True, 0.0), (33, 12.0, True, False, 0.0)]


@pytest.mark.parametrize("kind,hd", KIND_CASES)
@pytest.mark.parametrize("n,density,gaps,white,termination", RAY_CASES)
def test_ray_gradient_matches_autograd_of_the_definition(n, density, gaps, white, termination, kind, hd):
    delta, norm, lam_d, lam_e = 0.05, 7.0, 0.3, 0.02
    s, raw, index = _samples(n, 11 * n + int(white), density, gaps)
    target = np.array([0.2, 0.55, 0.9])
    ref = Q.ray_objective(s, raw, index, delta, target, float(white), termination, norm, kind, hd, lam_d, lam_e)
    kept = ref["kept"]
    if termination:
        assert 1 < kept < n, "the case is there for a cut"
    if density < 1e-3:
        assert ref["O"] < Q.CLAMP
    if density == 12.0:
        assert ref["O"] > 1 - Q.CLAMP
    if gaps and kept > 1:
        assert (np.diff(index[:kept]) > 1).any()
    ts, traw = torch.tensor(s, requires_grad=True), torch.tensor(raw, requires_grad=True)
    L, D, H = _torch_ray_loss(ts, traw, index, delta, target, float(white), kept, norm, kind, hd, lam_d, lam_e)
    L.backward()
    gs, graw = ts.grad.numpy()[:kept], traw.grad.numpy()[:kept]
    # D in prefix form is the O(S^2) definition, H the clamped entropy
    assert abs(ref["D"] - float(D.detach())) <= 1e-12 * max(float(D.detach()), 1e-30) + 1e-300
    assert abs(ref["D"] - Q.distortion_definition(ref["w"], (index[:kept] - index[0]) * delta, delta)) <= 1e-12 * max(ref["D"], 1e-30)
    assert abs(ref["H"] - float(H.detach())) <= 1e-14
    assert np.abs(gs).max() > 0
    assert np.abs(ref["ds"] - gs).max() <= 1e-10 * np.abs(gs).max(), (np.abs(ref["ds"] - gs).max(), np.abs(gs).max())
    assert np.abs(ref["draw"] - graw).max() <= 1e-10 * max(np.abs(graw).max(), 1e-300)
    assert (ts.grad.numpy()[kept:] == 0).all()
    # outside the entropy clamp only the distortion is left of the regularisers
    if density < 1e-3 or density == 12.0:
        off = Q.ray_objective(s, raw, index, delta, target, float(white), termination, norm, kind, hd, lam_d, 0.0)
        assert np.array_equal(off["ds"], ref["ds"])


RES = (4, 4, 3)
LO, HI = (-1.0, -1.0, -0.6), (1.0, 1.0, 0.6)
STEP = 0.07
FD_H = 1e-5


def _lattice_case(degree, dense=1.0):
    from tests.test_baked_train_host import _case
    return _case(degree, dense=dense)


@pytest.mark.parametrize("degree,white,termination,dense,kind,hd", [(0, False, 0.0, 1.0, Q.MSE, 0.0), (2, True, 0.0, 1.0, Q.HUBER, 0.3),
                                                                    (2, False, 0.05, 3.0, Q.LOG_COSH, 0.0), (0, True, 0.05, 3.0, Q.MAE, 0.0)])
def test_lattice_gradient_matches_autograd_and_central_differences(degree, white, termination, dense, kind, hd):
    sigma, co, o, d, near, far, target = _lattice_case(degree, dense)
    support = T.support_cells(sigma)
    lam_d, lam_e = 0.5, 0.05
    args = (LO, HI, o, d, near, far, STEP, target, support, white, termination, kind, hd, lam_d, lam_e)
    s64, co64 = sigma.astype(np.float64), co.astype(np.float64)
    info = {}
    L, terms, gs, gc = Q.loss_and_grad(s64, co64, *args, info=info)
    # the photometric part with mse and no regulariser is baked_train_reference's function
    if kind == Q.MSE:
        L0, _, gs0, gc0 = Q.loss_and_grad(s64, co64, *args[:11])
        Lt, gst, gct, _ = T.loss_and_grad(s64, co64, *args[:11])
        assert abs(L0 - Lt) <= 1e-15 and np.allclose(gs0, gst, rtol=0, atol=1e-16) and np.allclose(gc0, gct, rtol=0, atol=1e-16)
    assert abs(L - (terms["photometric"] + lam_d * terms["distortion"] + lam_e * terms["opacity_entropy"])) <= 1e-15
    raw, pre, Tn, opa = info["raw"], info["pre"], info["T"], info["opacity"]
    # preconditions: nothing on a kink
    assert np.abs(raw).min() > 1e-3 and np.abs(raw - 1).min() > 1e-3 and np.abs(pre).min() > 1e-3 and np.abs(pre - 1).min() > 1e-3
    diff = np.clip(pre, 0, 1) - target
    assert np.abs(diff).min() > 1e-3 and (kind != Q.HUBER or np.abs(np.abs(diff) - hd).min() > 1e-3)
    assert min(np.abs(opa - Q.CLAMP).min(), np.abs(opa - (1 - Q.CLAMP)).min()) > 1e-5
    if termination:
        assert (Tn < termination).sum() >= 3 and np.abs(Tn / termination - 1).min() > 1e-2
    assert (termination > 0 or info["gaps"].any()) and (info["kept"] > 0).all()
    # torch autograd of the definition through the same samples
    K = (degree + 1) ** 2
    ts = torch.tensor(s64.reshape(-1), requires_grad=True)
    tc = torch.tensor(co64.reshape(-1, K, 3), requires_grad=True)
    total = 0.0
    from tests import baked_reference as R
    for r in range(o.shape[0]):
        o64, d64 = o[r].astype(np.float64), d[r].astype(np.float64)
        idx, tau, index, nrm = Q.ray_geometry(RES, LO, HI, o64, d64, np.float64(near[r]), np.float64(far[r]), STEP, support)
        Y = torch.as_tensor(R.real_sh(d64 / nrm, degree, dtype=np.float64))
        tt = torch.as_tensor(tau)
        sj = (tt * ts[idx]).sum(1)
        raw_j = torch.einsum("mn,mnkc,k->mc", tt, tc[idx], Y)
        total = total + _torch_ray_loss(sj, raw_j, index, float(np.float32(STEP)) * nrm, target[r], float(white), int(info["kept"][r]),
                                        float(o.shape[0]), kind, hd, lam_d, lam_e)[0]
    total.backward()
    assert abs(float(total.detach()) - L) <= 1e-13
    ags, agc = ts.grad.numpy().reshape(RES), tc.grad.numpy().reshape(gc.shape)
    assert np.abs(gs - ags).max() <= 1e-10 * np.abs(ags).max() and np.abs(gc - agc).max() <= 1e-10 * np.abs(agc).max()
    # central differences of the reference's own loss
    worst = {"sigma": 0.0, "coef": 0.0}
    loss = lambda s, c: Q.loss_and_grad(s, c, *args)[0]
    rng = np.random.default_rng(5)
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


def test_float32_reference_and_the_total_minus_prefix_mirror():
    """the float32 form is the same function, and the kernel's summation order (total minus prefix) evaluates the same suffix"""
    s, raw, index = _samples(33, 3, 1.0, True)
    delta = 0.05
    ref = Q.ray_objective(s, raw, index, delta, np.zeros(3), 0.0, 0.0, 1.0, Q.MSE, 0.0, 1.0, 0.1)
    r32 = Q.ray_objective(s, raw, index, delta, np.zeros(3), 0.0, 0.0, 1.0, Q.MSE, 0.0, 1.0, 0.1, f=np.float32)
    assert r32["ds"].dtype == np.float32 and 0 < np.abs(r32["ds"] - ref["ds"]).max() < 1e-4 * np.abs(ref["ds"]).max()
    only = Q.ray_objective(s, np.full((33, 3), 0.5), index, delta, np.full(3, 0.5) * ref["O"], 0.0, 0.0, 1.0, Q.MSE, 0.0, 1.0, 0.1)
    assert only["sq"] < 1e-30                                              # no photometric part: ds is the regularisers' alone
    m = (index - index[0]) * delta
    _, dH = Q.entropy(ref["O"])
    for f, tol in ((np.float64, 1e-12), (np.float32, 1e-4)):
        mirror = Q.total_minus_prefix_mirror(ref["w"], m, delta, ref["T"], 1.0, 0.1 * dH, f)
        assert np.abs(mirror - only["ds"]).max() <= tol * np.abs(only["ds"]).max()


# ---- keywords
GOOD = [dict(loss="huber"), dict(loss="mae"), dict(loss="log_cosh"), dict(loss="mse"), dict(loss=None, regularizers=None),
        dict(loss={"class_name": "Huber", "config": {"delta": 0.1}}), dict(regularizers={"distortion": 0.01}),
        dict(regularizers={"distortion": 0.0, "opacity_entropy": 1e-3, "nets": "both"})]
BAD = [dict(loss="l1"), dict(loss=lambda a, b: 0), dict(loss={"class_name": "Huber", "config": {"delta": 0.0}}),
       dict(regularizers={"distortion": -1.0}), dict(regularizers={"opacity_entropy": float("nan")}), dict(regularizers=3),
       dict(regularizers={"distortion": 0.1, "nets": "fine"}), dict(regularizers={"nets": "coarse"}),
       dict(loss={"class_name": "Huber", "config": {"reduction": "sum"}})]


def _constructors():
    from keras_nerf_amd import baked_bricks_grow, baked_bricks_train, baked_train
    from keras_nerf_amd.baked import BakedField, BrickBakedField
    dense, brick = object.__new__(BakedField), object.__new__(BrickBakedField)      # no attribute: touching one is an AttributeError
    return [("BakedField.optimizer", BakedField.optimizer, dense), ("BakedFieldOptimizer", baked_train.BakedFieldOptimizer, dense),
            ("brick_optimizer", baked_train.brick_optimizer, brick), ("BrickFieldOptimizer", baked_bricks_train.BrickFieldOptimizer, brick),
            ("grid_trainer", baked_bricks_grow.grid_trainer, brick), ("BrickGridTrainer", baked_bricks_grow.BrickGridTrainer, brick)]


def test_every_constructor_takes_the_keywords_and_refuses_bad_values_first(monkeypatch):
    """accepted keywords get as far as the source field (an AttributeError of the attribute-less stand-in), bad values are a ValueError
    before that and before the library is touched"""
    from keras_nerf_amd import _lib, losses
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    for name, make, source in _constructors():
        sig = inspect.signature(make)
        assert sig.parameters["loss"].default is None and sig.parameters["regularizers"].default is None, name
        for kw in GOOD + [dict(loss=losses.Huber(0.1), regularizers=losses.RayRegularizers(distortion=0.01, opacity_entropy=1e-3))]:
            with pytest.raises(AttributeError):
                make(source, 0.05, 0.01, **kw)
        for kw in BAD:
            with pytest.raises(ValueError):
                make(source, 0.05, 0.01, **kw)
        with pytest.raises(ValueError, match="nets"):
            make(source, 0.05, 0.01, regularizers=losses.RayRegularizers(distortion=0.1, nets="fine"))


def test_check_objective_gives_the_record_or_none():
    from keras_nerf_amd import _lib, losses
    from keras_nerf_amd.baked_train import check_objective
    assert check_objective(None, None) is None and check_objective("mse", losses.RayRegularizers()) is None
    assert check_objective("mean_squared_error", {"distortion": 0.0, "opacity_entropy": 0.0}) is None
    obj = check_objective(losses.Huber(0.1), losses.RayRegularizers(distortion=0.01))
    assert losses.record_tuple(obj) == (_lib.LOSS_HUBER, pytest.approx(0.1), pytest.approx(0.01), 0.0, 3)
    assert check_objective("mse", {"opacity_entropy": 1e-3}).loss_kind == _lib.LOSS_MSE
    assert check_objective("mae", None).loss_kind == _lib.LOSS_MAE


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _bare(cls, objective):
    opt = object.__new__(cls)
    opt.field = types.SimpleNamespace(device=torch.device("cpu"), cell_size=(0.1, 0.1, 0.1))
    opt.step, opt.white_background, opt.termination, opt.lanes_per_ray = 0.05, False, 0.0, 0
    opt.objective, opt._terms, opt._c = objective, None, C.c_int(0)
    return opt


def test_the_plain_objective_calls_the_plain_entry_point(monkeypatch):
    from keras_nerf_amd import _lib, baked_bricks_grow, baked_bricks_train, baked_train
    from keras_nerf_amd.baked_train import check_objective
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(baked_train, "_stream", lambda dev: None)
    monkeypatch.setattr(baked_bricks_train, "_stream", lambda dev: None)
    o, d, tg = np.zeros((5, 3), np.float32), np.ones((5, 3), np.float32), np.zeros((5, 3), np.float32)
    for cls, plain_name in ((baked_train.BakedFieldOptimizer, "knerf_baked_train_rays"),
                            (baked_bricks_train.BrickFieldOptimizer, "knerf_baked_bricks_train_rays"),
                            (baked_bricks_grow.BrickGridTrainer, "knerf_baked_bricks_train_rays")):
        for kw in (dict(), dict(loss="mse"), dict(loss="mse", regularizers={"distortion": 0.0, "opacity_entropy": 0.0})):
            rec.calls.clear()
            opt = _bare(cls, check_objective(kw.get("loss"), kw.get("regularizers")))
            loss = opt.accumulate(o, d, 0.0, 1.0, tg)
            assert rec.calls == [plain_name], (cls.__name__, kw, rec.calls)
            assert loss.dtype == torch.float64 and opt.objective_terms() is None
        for kw in (dict(loss="huber"), dict(regularizers={"distortion": 0.01}), dict(loss="mse", regularizers={"opacity_entropy": 1e-3})):
            rec.calls.clear()
            opt = _bare(cls, check_objective(kw.get("loss"), kw.get("regularizers")))
            assert opt.objective_terms() is None
            loss = opt.accumulate(o, d, 0.0, 1.0, tg)
            assert rec.calls == [plain_name + "_ext"], (cls.__name__, kw, rec.calls)
            terms = opt.objective_terms()
            assert loss.dtype == torch.float64 and sorted(terms) == ["distortion", "mse", "opacity_entropy", "photometric"]
            assert all(v.dtype == torch.float64 and v.dim() == 0 for v in terms.values())


def test_the_new_symbols_are_declared_and_bound():
    import os
    import re
    from keras_nerf_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "knerf.h")).read()
    for name, plain in (("knerf_baked_train_rays_ext", "knerf_baked_train_rays"),
                        ("knerf_baked_bricks_train_rays_ext", "knerf_baked_bricks_train_rays")):
        assert re.search(r"\bint " + name + r"\(", header), name
        res, args = _lib.SIGNATURES[name]
        pres, pargs = _lib.SIGNATURES[plain]
        assert res is pres and args[:-2] == pargs and args[-2] is C.POINTER(_lib.KnerfObjective) and args[-1] is C.c_void_p


def test_ext_entry_points_refuse_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID decided on the host, no device needed: everything the plain twins refuse and the objective's own errors"""
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

    def obj(kind=_lib.LOSS_HUBER, delta=0.1, dist=0.01, ent=1e-3, nets=3):
        return _lib.KnerfObjective(kind, delta, dist, ent, nets)

    for fn, state in ((lib.knerf_baked_train_rays_ext, dense), (lib.knerf_baked_bricks_train_rays_ext, bricks)):
        def call(st, ob, o=p, target=p, n=10, n_norm=0, step=0.05, term=0.0, flags=0, terms=p):
            return fn(None, C.byref(st) if st is not None else None, o, p, None, None, 0.0, 1.0, target, n, n_norm, step, term, flags, None,
                      C.byref(ob) if ob is not None else None, terms)
        for ob in (None, obj(), obj(_lib.LOSS_MSE, 0.0, 0.0, 0.0)):
            assert call(state(), ob, n=0) == 0                             # no rays: nothing to launch, plain or extended
            assert call(None, ob) == INV
            for bad in (dict(records=None), dict(grad=None), dict(degree=4)):
                assert call(state(**bad), ob) == INV, bad
            for bad in (dict(o=None), dict(target=None), dict(step=0.0), dict(term=1.0), dict(flags=4), dict(flags=2 << 8), dict(n=1 << 36),
                        dict(n_norm=1 << 36)):
                assert call(state(), ob, **bad) == INV, bad
        for bad in (dict(kind=4), dict(kind=-1), dict(delta=0.0), dict(delta=-1.0), dict(delta=float("inf")), dict(delta=float("nan")),
                    dict(dist=-0.1), dict(dist=float("nan")), dict(dist=float("inf")), dict(ent=-1e-3), dict(ent=float("inf"))):
            assert call(state(), obj(**bad)) == INV, bad
            assert call(state(), obj(**bad), n=0) == INV, bad
        assert call(state(), obj(_lib.LOSS_MAE, delta=-1.0), n=0) == 0     # huber_delta is read under Huber only
        assert call(state(), obj(nets=0), n=0) == 0 and call(state(), obj(nets=77), n=0) == 0      # nets is ignored here
    assert lib.knerf_baked_train_rays_ext(None, C.byref(dense(n_slots=0)), p, p, None, None, 0.0, 1.0, p, 10, 0, 0.05, 0.0, 0, None,
                                          C.byref(obj()), p) == INV
    assert lib.knerf_baked_bricks_train_rays_ext(None, C.byref(bricks(log2=5)), p, p, None, None, 0.0, 1.0, p, 10, 0, 0.05, 0.0, 0, None,
                                                 C.byref(obj()), p) == INV
