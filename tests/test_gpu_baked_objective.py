"""The extended objective of the baked-field optimisers on the GPU (knerf_baked_train_rays_ext / knerf_baked_bricks_train_rays_ext behind
the loss= / regularizers= keywords) against tests/baked_objective_reference.py.  tests/README_baked_objective.md has the plan, the
bounds and what was measured.

Lattice, rays and seeds are those of tests/test_gpu_baked_train.py ((9, 7, 6) points, step 0.04, 150 rays, thin and opaque density).
Every case first asserts its preconditions on the fp64 reference alone: the clamp margins of that file, and for the new kinks (KINK =
1e-5, a hundred times the float32 error of a ray's output): no |d| of a ray that hit something within KINK of 0 under mae or of
huber_delta under Huber, no opacity within KINK / 10 of an edge of the entropy clamp; at least 20 % of the rays inside the entropy
clamp, a ray beyond each edge of it in the opaque cases without termination, a ray with exactly one fetched sample, one with none, and 5 % with a gap in
their fetched indices (with termination: three rays).

Bound per tensor and per term: max(1e-5 x max |fp64|, 4 x the deviation of the float32 run of the reference over 8 ray orders); with a
regulariser the float32 run is ALSO taken in the kernel's summation order (total minus prefix, Q.total_minus_prefix_mirror) and the
larger of the two deviations counts.  Measured on the CPU, never on the kernel."""
import numpy as np
import pytest
import torch

from tests import baked_objective_reference as Q
from tests import baked_train_reference as T
from tests import test_gpu_baked_train as B

pytestmark = pytest.mark.gpu

RES, LO, HI, STEP, N_RAYS = B.RES, B.LO, B.HI, B.STEP, B.N_RAYS
THIN, OPAQUE, TERMINATION, MARGIN = B.THIN, B.OPAQUE, B.TERMINATION, B.MARGIN
KINK = 1e-5
DIST, ENT = 0.5, 0.05
OBJECTIVES = {"mae": dict(loss_kind=Q.MAE), "huber": dict(loss_kind=Q.HUBER, huber_delta=0.05), "log_cosh": dict(loss_kind=Q.LOG_COSH),
              "mse+reg": dict(loss_kind=Q.MSE, distortion=DIST, opacity_entropy=ENT)}
NAMES = tuple(OBJECTIVES)
ENVS = ((THIN, False), (THIN, True), (OPAQUE, False), (OPAQUE, True))


def _keywords(name):
    from keras_nerf_amd import losses
    return {"mae": dict(loss="mae"), "huber": dict(loss=losses.Huber(0.05)), "log_cosh": dict(loss="log_cosh"),
            "mse+reg": dict(loss="mse", regularizers=losses.RayRegularizers(distortion=DIST, opacity_entropy=ENT)),
            "huber+reg": dict(loss=losses.Huber(0.1), regularizers=losses.RayRegularizers(distortion=1e-3, opacity_entropy=1e-4))}[name]


def _rays(degree):
    """the rays of tests/test_gpu_baked_train.py; four of those that start inside the box are moved into the dense part and end after
    one sample, so that a ray with exactly one fetched sample exists; one axis-parallel ray is shifted sideways (at degree 3 its opacity
    on the opaque lattice lay 4e-7 from the upper edge of the entropy clamp)"""
    rays = {k: v.copy() for k, v in B._rays(degree).items()}
    for i, at in zip(range(110, 114), ((-0.45, 0.2, 0.1), (-0.3, -0.35, 0.2), (-0.7, 0.3, -0.25), (0.05, -0.1, 0.3))):
        rays["o"][i], rays["near"][i], rays["far"][i] = at, 0.0, 0.03
    rays["o"][141] += np.where(rays["d"][141] == 0, np.float32(0.02), np.float32(0))
    return rays


_cases = {}


def _case(degree, dense, white, termination, name, own_target=False):
    """lattice, rays, the fp64 reference with its preconditions checked, and the bounds: computed once per case and shared.
    own_target: the target is the field's own image, so that every d is 0 and only the regularisers have a gradient"""
    key = (degree, dense, white, termination, name, own_target)
    if key in _cases:
        return _cases[key]
    sigma, co = B._lattice(degree, dense)
    rays = _rays(degree)
    support = T.support_cells(sigma)
    obj = OBJECTIVES[name]
    geo = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP)
    target = rays["target"]
    if own_target:
        probe = {}
        Q.loss_and_grad(*geo, target, support, white, termination, info=probe)
        target = probe["out"]                                              # float64: the reference's d is exactly 0
    args = geo + (target, support, white, termination)
    info = {}
    L, terms, gs, gc = Q.loss_and_grad(*args, **obj, info=info)
    raw, pre, opa, Tn, kept = info["raw"], info["pre"], info["opacity"], info["T"], info["kept"]
    hit = opa > 0
    assert min(np.abs(raw).min(), np.abs(raw - 1).min()) >= MARGIN, (key, "a raw colour on a clamp edge")
    assert min(np.abs(pre[hit]).min(), np.abs(pre[hit] - 1).min()) >= MARGIN, (key, "an output on a clamp edge")
    if termination:
        assert (Tn < termination).sum() >= 20 and np.abs(Tn / termination - 1).min() >= 1e-3, (key, "a transmittance on the threshold")
    d = np.abs(info["out"] - target)[hit]
    if own_target:
        assert (info["out"] == target).all() and terms["photometric"] == 0.0
    elif obj["loss_kind"] == Q.MAE:
        assert d.min() >= KINK, ("a difference on the kink of |d|", d.min())
    elif obj["loss_kind"] == Q.HUBER:
        assert np.abs(d - obj["huber_delta"]).min() >= KINK and (d > obj["huber_delta"]).any() and (d < obj["huber_delta"]).any(), \
            ("a difference on Huber's kink, or one branch unused", np.abs(d - obj["huber_delta"]).min())
    inside = (opa > Q.CLAMP) & (opa < 1 - Q.CLAMP)
    assert inside.mean() >= 0.2, inside.mean()
    assert min(np.abs(opa[hit] - Q.CLAMP).min(), np.abs(opa[hit] - (1 - Q.CLAMP)).min()) >= KINK / 10, (key, "an opacity on the entropy clamp")
    if dense == OPAQUE and not termination:                                # (a cut at 1e-2 leaves no opacity above 1 - 1e-4)
        assert (opa > 1 - Q.CLAMP).sum() >= 1 and (opa < Q.CLAMP).sum() >= 1, (key, "no ray beyond an edge of the entropy clamp")
    assert (kept == 1).sum() >= 1 and (kept == 0).sum() >= 1, (key, (kept == 1).sum(), (kept == 0).sum())
    # (a terminated ray often ends before the empty cells it would cross: there three rays with a gap are asked for)
    assert info["gaps"].mean() >= 0.05 or (termination and info["gaps"].sum() >= 3), (key, info["gaps"].mean())
    dev = {"gs": 0.0, "gc": 0.0, "L": 0.0, **{k: 0.0 for k in Q.TERMS}}
    rng = np.random.default_rng(99)
    regularised = obj.get("distortion", 0) > 0 or obj.get("opacity_entropy", 0) > 0
    for _ in range(8):                                                     # the fp32 reference's own error over 8 accumulation orders
        order = rng.permutation(N_RAYS)
        for mirror in ((False, True) if regularised else (False,)):
            L32, t32, s32, c32 = Q.loss_and_grad(*args, **obj, dtype=np.float32, order=order, mirror=mirror)
            dev["gs"], dev["gc"] = max(dev["gs"], float(np.abs(s32 - gs).max())), max(dev["gc"], float(np.abs(c32 - gc).max()))
            dev["L"] = max(dev["L"], abs(L32 - L))
            for k in Q.TERMS:
                dev[k] = max(dev[k], abs(t32[k] - terms[k]))
    ref = {"gs": gs, "gc": gc, "L": L, **terms}
    bound = {k: max(1e-5 * float(np.abs(ref[k]).max()), 4.0 * dev[k]) for k in dev}
    _cases[key] = {"sigma": sigma, "co": co, "rays": rays, "target": target, "support": support, "ref": ref, "bound": bound, "dev": dev,
                   "info": info}
    return _cases[key]


def _field(case):
    from keras_nerf_amd.baked import BakedField
    return BakedField.from_arrays(case["sigma"], case["co"], (LO, HI))


def _batch(case, sl=slice(None)):
    r = case["rays"]
    return r["o"][sl], r["d"][sl], r["near"][sl], r["far"][sl], np.asarray(case["target"], dtype=np.float32)[sl]


def _compare(opt, loss, case, what):
    """gradient, loss and the four terms of an accumulate() against the case's fp64 reference, each within its bound"""
    ref, bound = case["ref"], case["bound"]
    gs, gc = (g.cpu().numpy() for g in opt.gradients())
    got = {"gs": gs, "gc": gc, "L": float(loss), **{k: float(v) for k, v in opt.objective_terms().items()}}
    assert loss.dtype == torch.float64 and loss.dim() == 0
    slots = T.slot_points(case["support"])
    assert (gs[~slots] == 0).all() and (gc[~slots] == 0).all()
    line = []
    for k in bound:
        err = float(np.abs(got[k] - ref[k]).max())
        line.append(f"{k} {err:.3e} / {bound[k]:.3e} (fp32 {case['dev'][k]:.3e}, max {float(np.abs(ref[k]).max()):.3e})")
        assert err <= bound[k], (what, k, err, bound[k])
    print(f"{what}: error / bound  " + "; ".join(line))


# every (degree, objective) pair, the four environments dealt out so that every degree and every objective sees each of them; the
# regularised objective in all four environments at every degree; one terminated case per degree and objective
GRADIENT_CASES = sorted({(deg, *ENVS[(deg + k) % 4], 0.0, NAMES[k]) for deg in range(4) for k in range(4)} |
                        {(deg, *env, 0.0, "mse+reg") for deg in range(4) for env in ENVS} |
                        {(deg, OPAQUE, deg % 2 == 1, TERMINATION, NAMES[(deg + 1) % 4]) for deg in range(4)} |
                        {(2, OPAQUE, True, TERMINATION, "mse+reg")})


@pytest.mark.parametrize("degree,dense,white,termination,name", GRADIENT_CASES)
def test_gradient_and_terms_match_fp64(degree, dense, white, termination, name):
    case = _case(degree, dense, white, termination, name)
    for lanes in B.VARIANTS[degree]:
        opt = _field(case).optimizer(0.05, 0.01, step=STEP, white_background=white, termination=termination, lanes_per_ray=lanes,
                                     **_keywords(name))
        assert opt.objective_terms() is None
        loss = opt.accumulate(*_batch(case))
        _compare(opt, loss, case, f"degree {degree} dense {dense} white {white} termination {termination} {name} lanes {lanes}")


@pytest.mark.parametrize("degree,dense,white,termination", [(0, OPAQUE, False, 0.0), (1, THIN, True, 0.0), (2, OPAQUE, True, TERMINATION),
                                                            (3, THIN, False, 0.0)])
def test_regulariser_only_gradient(degree, dense, white, termination):
    """the target is the field's own image, rendered by the march the optimiser uses: every d is exactly 0, g is 0 on every channel and
    the gradient is the regularisers' alone -- a kernel that leaves at `g == 0` adds nothing"""
    case = _case(degree, dense, white, termination, "mse+reg", own_target=True)
    assert float(np.abs(case["ref"]["gs"]).max()) > 1e-7 and float(np.abs(case["ref"]["gc"]).max()) == 0.0
    rays = case["rays"]
    for lanes in B.VARIANTS[degree]:
        opt = _field(case).optimizer(0.05, 0.01, step=STEP, white_background=white, termination=termination, lanes_per_ray=lanes,
                                     **_keywords("mse+reg"))
        img = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, white_background=white, termination=termination,
                               lanes_per_ray=lanes, outputs="image")["image"]
        loss = opt.accumulate(rays["o"], rays["d"], rays["near"], rays["far"], img)
        terms = opt.objective_terms()
        assert float(terms["photometric"]) == 0.0 and float(terms["mse"]) == 0.0
        assert float(opt._grad[:, 1:].abs().max()) == 0.0 and float(opt._grad[:, 0].abs().max()) > 0.0
        _compare(opt, loss, case, f"regulariser only: degree {degree} dense {dense} white {white} termination {termination} lanes {lanes}")


def _one_ray_at_a_time(opt, case, n=N_RAYS, collect=None):
    o, d, near, far, tg = _batch(case)
    for r in range(n):
        loss = opt.accumulate(o[r:r + 1], d[r:r + 1], near[r:r + 1], far[r:r + 1], tg[r:r + 1], n_total=N_RAYS)
        if collect is not None:
            collect.append((loss, opt.objective_terms()))


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_the_extended_march_is_the_plain_march(degree):
    """Huber with delta = 2 and no regulariser where every |d| <= 1: rho = d^2 / 2, so every gradient row is exactly half the plain
    optimiser's, bit for bit (a factor of two is exact; one ray per launch fixes the order of the atomic adds)"""
    from keras_nerf_amd import losses
    for white in (False, True):
        case = _case(degree, THIN, white, 0.0, "huber")
        for lanes in B.VARIANTS[degree]:
            kw = dict(step=STEP, white_background=white, lanes_per_ray=lanes)
            plain = _field(case).optimizer(0.05, 0.01, **kw)
            ext = _field(case).optimizer(0.05, 0.01, loss=losses.Huber(2.0), **kw)
            _one_ray_at_a_time(plain, case)
            _one_ray_at_a_time(ext, case)
            g = plain._grad
            small = float(g[g != 0].abs().min())
            assert small > 1e-30 and int((g != 0).sum()) > 1000, small      # no denormal gradient: halving is exact
            assert torch.equal(ext._grad, 0.5 * g), (degree, white, lanes)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("b", [4, 8])
def test_bricks_equal_dense(degree, b):
    from keras_nerf_amd.baked_bricks_train import BRICK_TRAIN_VARIANTS
    from keras_nerf_amd.baked_train import brick_optimizer
    white = degree % 2 == 0
    case = _case(degree, THIN, white, 0.0, "mse+reg")
    bricks = _field(case).compact(b)
    dense = bricks.to_dense()
    for lanes in (0,) + BRICK_TRAIN_VARIANTS[degree]:
        kw = dict(step=STEP, white_background=white, lanes_per_ray=lanes, **_keywords("mse+reg"))
        D, S = dense.optimizer(0.05, 0.01, **kw), brick_optimizer(bricks, 0.05, 0.01, **kw)
        seen_d, seen_s = [], []
        _one_ray_at_a_time(D, case, collect=seen_d)
        _one_ray_at_a_time(S, case, collect=seen_s)
        for (ld, td), (ls, ts) in zip(seen_d, seen_s):
            assert torch.equal(ld, ls) and all(torch.equal(td[k], ts[k]) for k in td)
        for gd, gs in zip(D.gradients(), S.gradients()):
            assert torch.equal(gd, gs) and float(gd.abs().max()) > 0


@pytest.mark.parametrize("dilation", [0, 1])
def test_nothing_leaves_the_support(dilation):
    """ten steps with both regularisers and a sigma rate of 2: renders with and without skipping stay bit-identical, sigma stays
    exactly 0 outside the trainable points"""
    case = _case(2, THIN, False, 0.0, "mse+reg")
    rays = case["rays"]
    support = T.support_cells(case["sigma"], dilation)
    train = T.sigma_trainable(support)
    opt = _field(case).optimizer(2.0, 0.05, step=STEP, dilation=dilation, **_keywords("mse+reg"))
    assert np.array_equal(opt.sigma_trainable.cpu().numpy(), train)
    for k in range(10):
        opt.train_step(*_batch(case))
        a = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, skip_empty=True)
        c = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, skip_empty=False)
        for key in ("image", "depth", "opacity"):
            assert torch.equal(a[key], c[key]), (k, key)
    sigma = opt.field.sigma.cpu().numpy()
    assert (sigma[~train] == 0).all() and (sigma >= 0).all() and np.isfinite(sigma).all()
    assert np.abs(sigma[train] - case["sigma"][train]).max() > 1.0


def test_plain_stays_plain():
    """loss="mse" with RayRegularizers() is the optimiser without the keywords: records, moments and loss bit for bit"""
    from keras_nerf_amd import losses
    case = _case(2, THIN, True, 0.0, "mse+reg")
    a = _field(case).optimizer(0.05, 0.01, step=STEP, white_background=True)
    b = _field(case).optimizer(0.05, 0.01, step=STEP, white_background=True, loss="mse", regularizers=losses.RayRegularizers())
    assert b.objective is None
    for _ in range(3):
        la, lb = [], []
        _one_ray_at_a_time(a, case, collect=la)
        _one_ray_at_a_time(b, case, collect=lb)
        assert all(torch.equal(x[0], y[0]) and y[1] is None for x, y in zip(la, lb))
        assert torch.equal(a._grad, b._grad)
        a.apply(); b.apply()
        for x, y in ((a.field._records, b.field._records), (a._master, b._master), (a._m, b._m), (a._v, b._v)):
            assert torch.equal(x, y)
    assert b.objective_terms() is None


# final / initial objective (3.9455e-03 -> 2.0077e-04) of Q.optimise on the same 40 steps (huber 0.1, distortion 1e-3, opacity_entropy 1e-4), float64 on the CPU
REFERENCE_RATIO = 5.088e-2


def test_it_optimises():
    """tests/test_gpu_baked_train.py's optimisation under huber + both regularisers, through BakedFieldOptimizer and through
    grid_trainer: the GPU reaches at most twice the float64 NumPy optimiser's final / initial objective (the margin of that test)"""
    from keras_nerf_amd.baked import BakedField
    from keras_nerf_amd.baked_bricks_grow import grid_trainer
    sigma, co, rays, target = B._optimise_setup()
    start = BakedField.from_arrays(sigma, co, (LO, HI))
    batches = [(torch.as_tensor(target), (rays["o"], rays["d"], None))] * 40
    for opt in (start.optimizer(*B.OPT_RATES, step=STEP, **_keywords("huber+reg")),
                grid_trainer(start.compact(4), *B.OPT_RATES, step=STEP, **_keywords("huber+reg"))):
        hist = opt.fit(batches, rays["near"], rays["far"])
        final = float(opt.accumulate(rays["o"], rays["d"], rays["near"], rays["far"], target))
        assert len(hist["loss"]) == 40 and all(len(hist[k]) == 40 for k in Q.TERMS)
        assert abs(hist["loss"][3] - (hist["photometric"][3] + float(np.float32(1e-3)) * hist["distortion"][3] +
                                      float(np.float32(1e-4)) * hist["opacity_entropy"][3])) <= 1e-15     # (the record's weights are float32)
        ratio = final / hist["loss"][0]
        print(f"{type(opt).__name__}: objective {hist['loss'][0]:.4e} -> {final:.4e}: ratio {ratio:.4e} (reference {REFERENCE_RATIO})")
        assert ratio <= 2.0 * REFERENCE_RATIO


def test_ext_entry_points_refuse_bad_arguments_before_any_launch():
    """null and poisoned pointers: every call is refused on the host, before a launch could touch them"""
    import ctypes as C
    from keras_nerf_amd import _lib
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    p = C.c_void_p(4096)                                                  # never dereferenced: every call below is refused first
    field = _lib.KnerfBakedField(p, p, (C.c_int32 * 3)(*RES), 2, (C.c_float * 3)(*LO), (C.c_float * 3)(*HI))
    dense = _lib.KnerfBakedTrain(field, p, p, 10)
    bfield = _lib.KnerfBakedBricks(p, p, p, (C.c_int32 * 3)(*RES), 2, (C.c_float * 3)(*LO), (C.c_float * 3)(*HI), 2, 3)
    bricks = _lib.KnerfBakedBricksTrain(bfield, p)
    good = _lib.KnerfObjective(_lib.LOSS_HUBER, 0.1, 0.01, 1e-3, 3)
    for fn, st in ((lib.knerf_baked_train_rays_ext, dense), (lib.knerf_baked_bricks_train_rays_ext, bricks)):
        def call(ob, st=st, o=p, target=p, step=STEP, flags=0):
            return fn(None, C.byref(st) if st is not None else None, o, p, None, None, 0.0, 1.0, target, 10, 0, step, 0.0, flags, None,
                      C.byref(ob), p)
        for bad in ((4, 0.1, 0.0, 0.0), (-1, 0.1, 0.0, 0.0), (_lib.LOSS_HUBER, 0.0, 0.0, 0.0), (_lib.LOSS_HUBER, float("nan"), 0.0, 0.0),
                    (_lib.LOSS_MSE, 0.0, -1.0, 0.0), (_lib.LOSS_MSE, 0.0, float("inf"), 0.0), (_lib.LOSS_MAE, 0.0, 0.0, float("nan")),
                    (_lib.LOSS_MAE, 0.0, 0.0, -1e-3)):
            assert call(_lib.KnerfObjective(*bad, 3)) == INV, bad
        for kw in (dict(st=None), dict(o=None), dict(target=None), dict(step=0.0), dict(flags=4), dict(flags=2 << 8)):
            assert call(good, **kw) == INV, kw
    from keras_nerf_amd import losses
    case = _case(0, THIN, False, 0.0, "mae")
    for kw in (dict(loss="l1"), dict(regularizers=losses.RayRegularizers(distortion=0.1, nets="fine")), dict(regularizers={"distortion": -1})):
        with pytest.raises(ValueError):
            _field(case).optimizer(0.05, 0.01, **kw)
