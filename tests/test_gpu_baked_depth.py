"""Depth supervision of the baked-field optimisers on the GPU (knerf_baked_train_rays_depth / knerf_baked_bricks_train_rays_depth behind
the depth_loss= keyword and the depth= / depth_weight= arguments of accumulate()) against tests/baked_depth_reference.py, and the
sparse depth maps of the COLMAP loader against their closed form.

Lattice, rays and seeds are those of tests/test_gpu_baked_train.py ((9, 7, 6) points, step 0.04, 150 rays, thin and opaque density) with
the one-sample rays of tests/test_gpu_baked_objective.py; backgrounds and alphas those of tests/test_gpu_baked_rgba.py.  Depth targets:
z* = Z (1 + s u) around the fp64 reference's own depth Z, u in U(0.05, 0.3), s alternating in sign, a fixed positive value where Z = 0.
Weights: every third ray exactly 0 -- and its z* NaN, which pins the select --, every fifth (from 1) exactly 1, the rest in U(0.1, 2).
Every case first asserts its preconditions on the fp64 reference alone: those of test_gpu_baked_rgba.py, hit rays with Z > z* and with
Z < z*, hit rays with c = 0, and a one-sample ray and a no-sample ray with c > 0.

Bound per tensor and per term: max(1e-5 x max |fp64|, 4 x the deviation of the float32 run of the reference over 8 ray orders, in both
summation orders).  Measured on the CPU, never on the kernel.  No ray is left out of any comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import baked_depth_reference as D
from tests import baked_objective_reference as Q
from tests import baked_rgba_reference as P
from tests import baked_train_reference as T
from tests import test_gpu_baked_objective as O
from tests import test_gpu_baked_rgba as A
from tests import test_gpu_baked_train as B

pytestmark = pytest.mark.gpu

RES, LO, HI, STEP, N_RAYS = B.RES, B.LO, B.HI, B.STEP, B.N_RAYS
THIN, OPAQUE, TERMINATION, MARGIN, KINK = B.THIN, B.OPAQUE, B.TERMINATION, B.MARGIN, O.KINK
DIST, ENT, OPA, LAMZ = A.DIST, A.ENT, A.OPA, 0.2
Z_EMPTY = 2.5                      # the target of a ray whose reference depth is 0 (no fetched sample)
# name: (reference keywords, alpha targets, per-call backgrounds)
OBJECTIVES = {"mse+depth": (dict(loss_kind=Q.MSE, depth=LAMZ), False, False),
              "huber+reg+opacity+depth": (dict(loss_kind=Q.HUBER, huber_delta=0.05, distortion=DIST, opacity_entropy=ENT, opacity=OPA,
                                               depth=LAMZ), True, True),
              "mae+background+depth": (dict(loss_kind=Q.MAE, depth=LAMZ), False, True)}
NAMES = tuple(OBJECTIVES)
ENVS = A.ENVS


def _keywords(name, depth_loss=LAMZ):
    from keras_nerf_amd import losses
    return {"mse+depth": dict(depth_loss=depth_loss),
            "huber+reg+opacity+depth": dict(loss=losses.Huber(0.05), regularizers=losses.RayRegularizers(distortion=DIST, opacity_entropy=ENT),
                                            opacity_loss=OPA, depth_loss=depth_loss),
            "mae+background+depth": dict(loss="mae", depth_loss=depth_loss)}[name]


def _depth_inputs(Z, seed):
    """(z* [N], c [N]) float32 around the reference depths Z"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.05, 0.3, N_RAYS)
    s = np.where(np.arange(N_RAYS) % 2 == 0, 1.0, -1.0)
    z = np.where(Z > 0, Z * (1.0 + s * u), Z_EMPTY).astype(np.float32)
    c = rng.uniform(0.1, 2.0, N_RAYS).astype(np.float32)
    c[1::5] = 1.0
    c[::3] = 0.0                                                           # (after the ones: EVERY third ray has weight 0)
    z[c == 0] = np.nan
    return z, c


_cases = {}


def _case(degree, dense, termination, name, stored, mode="mixed", seed=11):
    """lattice, rays, backgrounds, alphas, depth targets and weights, the fp64 reference with its preconditions checked, and the bounds:
    computed once per case.  mode "own": the target is the reference's own output, so every d is exactly 0 and only the depth term has
    a gradient"""
    key = (degree, dense, termination, name, stored, mode)
    if key in _cases:
        return _cases[key]
    sigma, co = B._lattice(degree, dense)
    rays = O._rays(degree)
    support = T.support_cells(sigma)
    obj, with_alpha, with_bg = OBJECTIVES[name]
    bg, alpha = (A._backgrounds() if with_bg else None), (A._alphas() if with_alpha else None)
    geo = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP)
    target = rays["target"]
    probe = {}
    D.loss_and_grad(*geo, target, support, background=bg, termination=termination, info=probe)
    if mode == "own":
        target = probe["out"]                                              # float64: the reference's d is exactly 0
    z, c = _depth_inputs(probe["Z"], seed)
    kw = dict(background=bg, alpha=alpha, stored=stored, termination=termination, depth_target=z, depth_weight=c, **obj)
    args = geo + (target, support)
    info = {}
    L, terms, gs, gc = D.loss_and_grad(*args, **kw, info=info)
    raw, pre, opa, Tn, kept, Z = info["raw"], info["pre"], info["opacity"], info["T"], info["kept"], info["Z"]
    hit = opa > 0
    bgs = np.zeros((N_RAYS, 3)) if bg is None else bg
    # the preconditions of tests/test_gpu_baked_rgba.py
    assert min(np.abs(raw).min(), np.abs(raw - 1).min()) >= MARGIN, (key, "a raw colour on a clamp edge")
    assert min(np.abs(pre[hit]).min(), np.abs(pre[hit] - 1).min()) >= MARGIN, (key, "an output on a clamp edge")
    assert (pre[~hit] == bgs[~hit]).all()
    if termination:
        assert (Tn < termination).sum() >= 20 and np.abs(Tn / termination - 1).min() >= 1e-3, (key, "a transmittance on the threshold")
    d = np.abs(info["out"] - info["tgt"])
    if mode == "own":
        assert (info["out"] == info["tgt"]).all() and terms["photometric"] == 0.0
    elif obj["loss_kind"] == Q.MAE:
        assert d.min() >= KINK, ("a difference on the kink of |d|", d.min())
    elif obj["loss_kind"] == Q.HUBER:
        assert np.abs(d - obj["huber_delta"]).min() >= KINK and (d > obj["huber_delta"]).any() and (d < obj["huber_delta"]).any(), \
            ("a difference on Huber's kink, or one branch unused", np.abs(d - obj["huber_delta"]).min())
    inside = (opa > Q.CLAMP) & (opa < 1 - Q.CLAMP)
    assert inside.mean() >= 0.2, inside.mean()
    assert min(np.abs(opa[hit] - Q.CLAMP).min(), np.abs(opa[hit] - (1 - Q.CLAMP)).min()) >= KINK / 10, (key, "an opacity on the entropy clamp")
    if dense == OPAQUE and not termination:
        assert (opa > 1 - Q.CLAMP).sum() >= 1 and (opa < Q.CLAMP).sum() >= 1, (key, "no ray beyond an edge of the entropy clamp")
    assert (kept == 1).sum() >= 1 and (kept == 0).sum() >= 1, (key, (kept == 1).sum(), (kept == 0).sum())
    assert info["gaps"].mean() >= 0.05 or (termination and info["gaps"].sum() >= 3), (key, info["gaps"].mean())
    if alpha is not None:
        assert (hit & (alpha == 0)).any() and (hit & (alpha == 1)).any(), (key, "no hit ray with alpha 0 or 1")
        assert (hit & (opa > alpha)).any() and (hit & (opa < alpha)).any(), (key, "the opacities lie on one side of alpha")
    # ... and those of the depth term
    live = c > 0
    assert np.array_equal(Z, probe["Z"]) and (Z[hit] > 0).all() and (Z[~hit] == 0).all()
    assert np.isnan(z[~live]).all() and np.isfinite(z[live]).all() and (c == 1).sum() >= 20 and (~live).sum() == 50
    assert (hit & live & (Z > z)).sum() >= 10 and (hit & live & (Z < z)).sum() >= 10, (key, "the depths lie on one side of their targets")
    assert (hit & ~live).sum() >= 10, (key, "no hit ray of weight 0")
    assert ((kept == 1) & live).any() and ((kept == 0) & live).any(), (key, "no one-sample or no-sample ray of weight > 0")
    assert (info["zterm"][~live] == 0).all() and np.allclose(info["zterm"][(kept == 0) & live], c[(kept == 0) & live] * Z_EMPTY ** 2)
    assert np.isfinite(L) and np.isfinite(gs).all() and np.isfinite(gc).all() and terms["depth"] > 0
    names = ("gs", "gc", "L") + D.TERMS
    dev = {k: 0.0 for k in names}
    rng = np.random.default_rng(99)
    for _ in range(8):                                                     # the fp32 reference's own error over 8 accumulation orders
        order = rng.permutation(N_RAYS)
        for mirror in (False, True):
            L32, t32, s32, c32 = D.loss_and_grad(*args, **kw, dtype=np.float32, order=order, mirror=mirror)
            dev["gs"], dev["gc"] = max(dev["gs"], float(np.abs(s32 - gs).max())), max(dev["gc"], float(np.abs(c32 - gc).max()))
            dev["L"] = max(dev["L"], abs(L32 - L))
            for k in D.TERMS:
                dev[k] = max(dev[k], abs(t32[k] - terms[k]))
    ref = {"gs": gs, "gc": gc, "L": L, **terms}
    bound = {k: max(1e-5 * float(np.abs(ref[k]).max()), 4.0 * dev[k]) for k in dev}
    _cases[key] = {"sigma": sigma, "co": co, "rays": rays, "target": target, "support": support, "bg": bg, "alpha": alpha, "stored": stored,
                   "z": z, "c": c, "ref": ref, "bound": bound, "dev": dev, "info": info, "kw": kw, "args": args}
    return _cases[key]


_field, _target, _target_background = A._field, A._target, A._target_background


def _batch(case, sl=slice(None)):
    r = case["rays"]
    return r["o"][sl], r["d"][sl], r["near"][sl], r["far"][sl], _target(case, sl)


def _extra(case, sl=slice(None), depth=True):
    out = {} if case["bg"] is None else dict(background=case["bg"][sl])
    if depth:
        out.update(depth=case["z"][sl], depth_weight=case["c"][sl])
    return out


def _compare(opt, loss, case, what):
    """gradient, loss and the six terms of an accumulate() against the case's fp64 reference, each within its bound"""
    ref, bound = case["ref"], case["bound"]
    gs, gc = (g.cpu().numpy() for g in opt.gradients())
    got = {"gs": gs, "gc": gc, "L": float(loss), **{k: float(v) for k, v in opt.objective_terms().items()}}
    assert loss.dtype == torch.float64 and loss.dim() == 0 and tuple(opt.objective_terms()) == D.TERMS
    assert np.isfinite(gs).all() and np.isfinite(gc).all() and np.isfinite(got["L"])          # the NaN targets of weight 0 went nowhere
    slots = T.slot_points(case["support"])
    assert (gs[~slots] == 0).all() and (gc[~slots] == 0).all()
    line = []
    for k in bound:
        err = float(np.abs(got[k] - ref[k]).max())
        line.append(f"{k} {err:.3e} / {bound[k]:.3e} (fp32 {case['dev'][k]:.3e}, max {float(np.abs(ref[k]).max()):.3e})")
        assert err <= bound[k], (what, k, err, bound[k])
    print(f"{what}: error / bound  " + "; ".join(line))


# every (degree, objective) pair; the three environments dealt out so that every degree and every objective sees each of them
GRADIENT_CASES = [(deg, *ENVS[(deg + k) % 3], NAMES[k], float((deg + k) % 2)) for deg in range(4) for k in range(3)]


@pytest.mark.parametrize("degree,dense,termination,name,stored", GRADIENT_CASES)
def test_gradient_and_terms_match_fp64(degree, dense, termination, name, stored):
    """dense and bricks (compact(4)), every lane variant"""
    from keras_nerf_amd.baked_bricks_train import BRICK_TRAIN_VARIANTS
    from keras_nerf_amd.baked_train import brick_optimizer
    case = _case(degree, dense, termination, name, stored)
    kw = dict(step=STEP, termination=termination, target_background=_target_background(stored), **_keywords(name))
    what = f"degree {degree} dense {dense} termination {termination} {name} stored {stored}"
    for lanes in B.VARIANTS[degree]:
        opt = _field(case).optimizer(0.05, 0.01, lanes_per_ray=lanes, **kw)
        assert opt.objective_terms() is None and opt.depth_loss == LAMZ
        loss = opt.accumulate(*_batch(case), **_extra(case))
        _compare(opt, loss, case, f"{what} lanes {lanes}")
    bricks = _field(case).compact(4)
    for lanes in (0,) + BRICK_TRAIN_VARIANTS[degree]:
        opt = brick_optimizer(bricks, 0.05, 0.01, lanes_per_ray=lanes, **kw)
        loss = opt.accumulate(*_batch(case), **_extra(case))
        _compare(opt, loss, case, f"{what} bricks lanes {lanes}")


@pytest.mark.parametrize("degree,dense,termination", [(0, OPAQUE, 0.0), (1, THIN, 0.0), (2, OPAQUE, TERMINATION), (3, THIN, 0.0)])
def test_depth_only_gradient(degree, dense, termination):
    """the target is the field's own image, rendered by the march the optimiser uses: every d is exactly 0, g is 0 on every channel and
    the gradient is the depth term's alone -- a kernel that leaves at `g == 0` without looking at the depth weight adds nothing"""
    case = _case(degree, dense, termination, "mse+depth", 0.0, mode="own")
    assert float(np.abs(case["ref"]["gs"]).max()) > 1e-7 and float(np.abs(case["ref"]["gc"]).max()) == 0.0
    rays = case["rays"]
    for lanes in B.VARIANTS[degree]:
        opt = _field(case).optimizer(0.05, 0.01, step=STEP, termination=termination, lanes_per_ray=lanes, depth_loss=LAMZ)
        img = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, termination=termination, lanes_per_ray=lanes,
                               outputs="image")["image"]
        loss = opt.accumulate(rays["o"], rays["d"], rays["near"], rays["far"], img, depth=case["z"], depth_weight=case["c"])
        terms = opt.objective_terms()
        assert float(terms["photometric"]) == 0.0 and float(terms["mse"]) == 0.0 and float(terms["depth"]) > 0.0
        assert float(opt._grad[:, 1:].abs().max()) == 0.0 and float(opt._grad[:, 0].abs().max()) > 0.0
        _compare(opt, loss, case, f"depth only: degree {degree} dense {dense} termination {termination} lanes {lanes}")


def _one_ray_at_a_time(opt, case, collect=None, n_total=N_RAYS, depth=None, depth_weight=None):
    """one ray per launch fixes the order of the atomic adds; depth / depth_weight: [N] arrays or None"""
    o, d, near, far, tg = _batch(case)
    for r in range(N_RAYS):
        extra = _extra(case, slice(r, r + 1), depth=False)
        if depth is not None:
            extra["depth"] = depth[r:r + 1]
        if depth_weight is not None:
            extra["depth_weight"] = depth_weight[r:r + 1]
        loss = opt.accumulate(o[r:r + 1], d[r:r + 1], near[r:r + 1], far[r:r + 1], tg[r:r + 1], n_total=n_total, **extra)
        if collect is not None:
            collect.append((loss, opt.objective_terms()))


FULL = "huber+reg+opacity+depth"


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_no_weight_is_no_depth_bit_for_bit(degree):
    """(a) depth_loss = 0 with depth tensors given is the launch without the keyword; depth_loss > 0 with every weight 0 (and every target
    NaN) runs the depth kernel and adds the same bits: gradient rows, loss and the first five terms"""
    case = _case(degree, THIN, 0.0, FULL, 0.0)
    nan, zero = np.full(N_RAYS, np.nan, np.float32), np.zeros(N_RAYS, np.float32)
    for lanes in B.VARIANTS[degree]:
        make = lambda z: _field(case).optimizer(0.05, 0.01, step=STEP, lanes_per_ray=lanes, target_background="black", **_keywords(FULL, z))
        kw = _keywords(FULL)
        del kw["depth_loss"]
        plain = _field(case).optimizer(0.05, 0.01, step=STEP, lanes_per_ray=lanes, target_background="black", **kw)
        off, weightless = make(0.0), make(LAMZ)
        seen = [[], [], []]
        _one_ray_at_a_time(plain, case, collect=seen[0])
        _one_ray_at_a_time(off, case, collect=seen[1], depth=case["z"], depth_weight=case["c"])
        _one_ray_at_a_time(weightless, case, collect=seen[2], depth=nan, depth_weight=zero)
        assert tuple(seen[0][0][1]) == tuple(seen[1][0][1]) == P.TERMS and tuple(seen[2][0][1]) == D.TERMS
        A._same(seen[0], seen[1], P.TERMS)
        A._same(seen[0], seen[2], P.TERMS)
        assert all(float(t["depth"]) == 0.0 for _, t in seen[2])
        assert torch.equal(plain._grad, off._grad) and torch.equal(plain._grad, weightless._grad) and float(plain._grad.abs().max()) > 0


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("dense,termination", [(THIN, 0.0), (OPAQUE, TERMINATION)])
def test_the_depth_is_the_rendered_depth_bit_for_bit(degree, dense, termination):
    """(b) with z* = 0 and c = 1, one ray per launch and n_total = 1, the depth term is float32(D) float32(D) with D the depth the live
    field's render writes for that ray (same step, termination, lane variant, empty cells skipped over the support);
    (c) with z* = that D the depth term is exactly 0 and the gradient rows are those of the run without depth, bit for bit"""
    case = _case(degree, dense, termination, FULL, 0.0)
    rays = case["rays"]
    kw = _keywords(FULL)
    del kw["depth_loss"]
    for lanes in B.VARIANTS[degree]:
        common = dict(step=STEP, termination=termination, lanes_per_ray=lanes, target_background="black")
        opt = _field(case).optimizer(0.05, 0.01, depth_loss=LAMZ, **common)
        depth = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, termination=termination, lanes_per_ray=lanes,
                                 outputs="depth", skip_empty=True)["depth"].cpu().numpy()
        assert depth.dtype == np.float32 and (depth > 0).sum() >= 90
        seen = []
        o, d, near, far, tg = _batch(case)
        for r in range(N_RAYS):
            opt.accumulate(o[r:r + 1], d[r:r + 1], near[r:r + 1], far[r:r + 1], tg[r:r + 1, :3], n_total=1, depth=np.zeros(1, np.float32))
            seen.append(float(opt.objective_terms()["depth"]))
        want = (depth * depth).astype(np.float64)                          # the product in float32
        assert np.array_equal(np.array(seen), want), (degree, lanes, np.abs(np.array(seen) - want).max())
        without = _field(case).optimizer(0.05, 0.01, **common, **kw)
        onto = _field(case).optimizer(0.05, 0.01, depth_loss=LAMZ, **common, **kw)
        seen_w, seen_o = [], []
        _one_ray_at_a_time(without, case, collect=seen_w)
        _one_ray_at_a_time(onto, case, collect=seen_o, depth=depth, depth_weight=case["c"])
        A._same(seen_w, seen_o, P.TERMS)
        assert all(float(t["depth"]) == 0.0 for _, t in seen_o)
        assert torch.equal(without._grad, onto._grad) and float(onto._grad.abs().max()) > 0, (degree, lanes)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("b", [4, 8])
def test_bricks_equal_dense(degree, b):
    """(d) under the full objective with depth, bit for bit"""
    from keras_nerf_amd.baked_bricks_train import BRICK_TRAIN_VARIANTS
    from keras_nerf_amd.baked_train import brick_optimizer
    stored = float(degree % 2)
    case = _case(degree, THIN, 0.0, FULL, stored)
    bricks = _field(case).compact(b)
    dense = bricks.to_dense()
    for lanes in (0,) + BRICK_TRAIN_VARIANTS[degree]:
        kw = dict(step=STEP, lanes_per_ray=lanes, target_background=_target_background(stored), **_keywords(FULL))
        Dn, S = dense.optimizer(0.05, 0.01, **kw), brick_optimizer(bricks, 0.05, 0.01, **kw)
        seen_d, seen_s = [], []
        _one_ray_at_a_time(Dn, case, collect=seen_d, depth=case["z"], depth_weight=case["c"])
        _one_ray_at_a_time(S, case, collect=seen_s, depth=case["z"], depth_weight=case["c"])
        A._same(seen_d, seen_s, D.TERMS)
        assert any(float(t["depth"]) > 0 for _, t in seen_d)
        for gd, gs in zip(Dn.gradients(), S.gradients()):
            assert torch.equal(gd, gs) and float(gd.abs().max()) > 0


STEPS = 3


def _per_step(case):
    """what one Adam step can add to the difference between the GPU's objective and the reference's (the reasoning stands in
    test_three_steps_track_the_reference)"""
    n_par = int(T.slot_points(case["support"]).sum()) * (1 + 3 * case["co"].shape[3])
    e_g = max(case["bound"]["gs"], case["bound"]["gc"])
    ulp16 = float(np.spacing(np.float16(np.abs(case["co"].astype(np.float32)).max())))
    return n_par * 2.0 * max(B.OPT_RATES) * e_g + 2.0 * float(np.abs(case["ref"]["gc"]).max()) * ulp16


def test_three_steps_track_the_reference():
    """Three full-batch Adam steps of the dense optimiser, the brick optimiser and the grid trainer under mse + depth against
    D.optimise(): the objective before every step and after the last.
    Tolerance of value k (k steps taken): the case's bound of L at the start, plus k times what one step can add.  A step moves a
    parameter by at most its bias-corrected rate, and the move differs between fp32 and fp64 gradients by at most twice that only
    where the gradient is no larger than its fp32 error e_g (elsewhere Adam's quotient agrees to rounding): to first order the
    objective then differs by at most n_parameters x 2 rate x e_g; e_g is the gradient bound of the case.  A master value that
    rounds to another fp16 neighbour than the reference's (the two masters differ by fp32 rounding, 2^-13 of an fp16 step, so a
    handful of the 10^4 parameters per step) moves the objective by at most max |g_coef| x ulp16(max |coefficient|); two are allowed."""
    from keras_nerf_amd.baked_bricks_grow import grid_trainer
    from keras_nerf_amd.baked_train import brick_optimizer
    case = _case(2, THIN, 0.0, "mse+depth", 0.0)
    rays = case["rays"]
    want = D.optimise(case["sigma"], case["co"], LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP, case["target"],
                      *B.OPT_RATES, STEPS, depth_target=case["z"], depth_weight=case["c"], depth=LAMZ)
    assert len(want) == STEPS + 1 and want[-1] < want[0]
    per_step = _per_step(case)
    start = _field(case)
    batch = _batch(case)
    for build in (lambda **kw: start.optimizer(*B.OPT_RATES, step=STEP, **kw), lambda **kw: brick_optimizer(start.compact(4), *B.OPT_RATES, step=STEP, **kw),
                  lambda **kw: grid_trainer(start.compact(4), *B.OPT_RATES, step=STEP, **kw)):
        opt = build(depth_loss=LAMZ)
        got = [float(opt.train_step(*batch, depth=case["z"], depth_weight=case["c"])) for _ in range(STEPS)]
        got.append(float(opt.accumulate(*batch, depth=case["z"], depth_weight=case["c"])))
        assert opt.iterations == STEPS
        for k, (g, w) in enumerate(zip(got, want)):
            tol = case["bound"]["L"] + k * per_step
            print(f"{type(opt).__name__} after {k} steps: objective {g:.9e}, reference {w:.9e}, error {abs(g - w):.3e} / {tol:.3e}")
            assert abs(g - w) <= tol, (type(opt).__name__, k, abs(g - w), tol)


def test_depth_entry_points_refuse_bad_arguments_before_any_launch():
    """on live optimisers with valid device pointers: every bad record is refused and the gradient buffer stays zero"""
    from keras_nerf_amd import _lib
    from keras_nerf_amd.baked import _check, _stream
    from keras_nerf_amd.baked_train import brick_optimizer
    from keras_nerf_amd.runtime import _f32, _ptr
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    case = _case(2, THIN, 0.0, FULL, 0.0)
    o, d, near, far, tg = (_f32(x, "cuda") for x in _batch(case))
    rgb, alpha, bg = tg[:, :3].contiguous(), tg[:, 3].contiguous(), _f32(case["bg"], "cuda")
    z, c = _f32(np.nan_to_num(case["z"], nan=1.0), "cuda"), _f32(case["c"], "cuda")
    terms = torch.zeros((N_RAYS, 6), device="cuda")
    sq = torch.zeros((N_RAYS,), device="cuda")
    huber = _lib.KnerfObjective(_lib.LOSS_HUBER, 0.1, 0.01, 1e-3, 3)
    for opt, fn, name in ((_field(case).optimizer(0.05, 0.01, step=STEP), lib.knerf_baked_train_rays_depth, "knerf_baked_train_rays_depth"),
                          (brick_optimizer(_field(case).compact(4), 0.05, 0.01, step=STEP), lib.knerf_baked_bricks_train_rays_depth,
                           "knerf_baked_bricks_train_rays_depth")):
        terms.zero_()

        def call(rec, ob=None, rg=None, step=STEP, fl=_lib.BAKED_SKIP_EMPTY, target=rgb):
            return fn(_stream(o.device), C.byref(opt._c), _ptr(o), _ptr(d), _ptr(near), _ptr(far), 0.0, 0.0, _ptr(target), N_RAYS, 0, step, 0.0,
                      fl, _ptr(sq), C.byref(ob) if ob is not None else None, _ptr(terms), C.byref(rg) if rg is not None else None,
                      C.byref(rec) if rec is not None else None)
        Z_, C_ = z.data_ptr(), c.data_ptr()
        good_rgba = _lib.KnerfBakedRgba(bg.data_ptr(), alpha.data_ptr(), 0.0, 0.1)
        for bad in ((Z_, C_, -0.1), (Z_, C_, float("nan")), (Z_, C_, float("inf")), (Z_, None, -1.0), (None, C_, 0.1), (None, None, 1e-3)):
            for ob in (None, huber):
                for rg in (None, good_rgba):
                    rc = call(_lib.KnerfBakedDepth(*bad), ob, rg)
                    assert rc == INV, bad
                    with pytest.raises(ValueError, match=f"{name} refused its arguments"):
                        _check(rc, name)
        good = _lib.KnerfBakedDepth(Z_, C_, 0.1)
        # everything the _rgba entry point refuses, with a good depth record behind it
        for bad in ((bg.data_ptr(), alpha.data_ptr(), 0.5, 0.1), (bg.data_ptr(), alpha.data_ptr(), 0.0, -0.1), (bg.data_ptr(), None, 0.0, 0.1)):
            assert call(good, None, _lib.KnerfBakedRgba(*bad)) == INV, bad
        assert call(good, _lib.KnerfObjective(7, 0.1, 0.0, 0.0, 3)) == INV and call(good, _lib.KnerfObjective(_lib.LOSS_MSE, 0.0, -1.0, 0.0, 3)) == INV
        assert call(good, step=0.0) == INV and call(good, fl=4) == INV and call(good, fl=2 << 8) == INV and call(good, target=None) == INV
        torch.cuda.synchronize()
        assert float(opt._grad.abs().max()) == 0.0 and float(terms.abs().max()) == 0.0
        assert call(good, huber, good_rgba) == 0
        torch.cuda.synchronize()
        assert float(opt._grad.abs().max()) > 0.0 and float(terms[:, 5].max()) > 0.0
        # a NULL record and a weight of 0 are the _rgba call: terms keeps that route's stride of 5
        for off in (None, _lib.KnerfBakedDepth(None, None, 0.0)):
            terms.zero_()
            assert call(off, huber, good_rgba) == 0
            torch.cuda.synchronize()
            flat = terms.reshape(-1)
            assert float(flat[:5 * N_RAYS].abs().max()) > 0.0 and float(flat[5 * N_RAYS:].abs().max()) == 0.0


def test_the_python_surface_refuses():
    from keras_nerf_amd.baked_bricks_grow import grid_trainer
    from keras_nerf_amd.baked_train import brick_optimizer, fit_coarse_to_fine
    case = _case(2, THIN, 0.0, "mse+depth", 0.0)
    field = _field(case)
    for bad in (-0.1, float("nan"), float("inf"), "1", True, 1e39):
        for make in (lambda **kw: field.optimizer(0.05, 0.01, **kw), lambda **kw: brick_optimizer(field.compact(4), 0.05, 0.01, **kw),
                     lambda **kw: grid_trainer(field.compact(4), 0.05, 0.01, **kw)):
            with pytest.raises(ValueError, match="depth_loss"):
                make(depth_loss=bad)
        with pytest.raises(ValueError, match="depth_loss"):
            fit_coarse_to_fine(field, [], 0.0, 1.0, [(None, 1)], learning_rate_sigma=0.05, learning_rate_sh=0.01, depth_loss=bad)
    opt = field.optimizer(0.05, 0.01, step=STEP, depth_loss=LAMZ)
    o, d, near, far, tg = _batch(case)
    with pytest.raises(ValueError, match="depth_loss > 0 needs depth"):
        opt.accumulate(o, d, near, far, tg)
    with pytest.raises(ValueError, match="depth_loss > 0 needs depth"):
        opt.train_step(o, d, near, far, tg, depth_weight=case["c"])
    for bad in (dict(depth=case["z"][:5]), dict(depth=case["z"], depth_weight=case["c"][:5]), dict(depth=case["z"][:, None])):
        with pytest.raises(ValueError, match=r"must be \[150\]"):
            opt.accumulate(o, d, near, far, tg, **bad)
    assert float(opt._grad.abs().max()) == 0.0 and opt.objective_terms() is None
    with pytest.raises(ValueError, match="QuantizedBrickField"):
        brick_optimizer(field.compact(4).quantize(), 0.05, 0.01, depth_loss=LAMZ)
    with pytest.raises(ValueError, match="QuantizedBrickField"):
        grid_trainer(field.compact(4).quantize(), 0.05, 0.01, depth_loss=LAMZ)


def test_fit_passes_the_batches_depth_on():
    """fit() reads last_depth after each batch is drawn; fit_coarse_to_fine hands it through its stages"""
    from keras_nerf_amd.baked_train import fit_coarse_to_fine
    case = _case(2, THIN, 0.0, "mse+depth", 0.0)
    o, d, near, far, tg = _batch(case)

    class Batches:
        last_depth = None

        def __iter__(self):
            for _ in range(2):
                self.last_depth = (torch.as_tensor(case["z"]).cuda(), torch.as_tensor(case["c"]).cuda())
                yield torch.as_tensor(tg), (o, d, None)

    opt = _field(case).optimizer(*B.OPT_RATES, step=STEP, depth_loss=LAMZ)
    hist = opt.fit(Batches(), near, far)
    ref = _field(case).optimizer(*B.OPT_RATES, step=STEP, depth_loss=LAMZ)
    want = [float(ref.train_step(o, d, near, far, tg, depth=case["z"], depth_weight=case["c"])) for _ in range(2)]
    # the first value is the same launch on the same records; the second follows a step whose gradient the atomic adds summed in
    # another order: within the tolerance of one step, twice (either run against the reference)
    assert hist["loss"][0] == want[0] and abs(hist["loss"][1] - want[1]) <= 2.0 * (case["bound"]["L"] + _per_step(case))
    assert list(hist) == ["loss"] + list(D.TERMS) and all(v > 0 for v in hist["depth"]) and opt.iterations == 2
    _, history = fit_coarse_to_fine(_field(case), Batches(), near, far, [(None, 1), (None, 1)], learning_rate_sigma=B.OPT_RATES[0],
                                    learning_rate_sh=B.OPT_RATES[1], step=STEP, depth_loss=LAMZ)
    assert history["loss"][0] == want[0] and len(history["depth"]) == 2 and [s["steps"] for s in history["stages"]] == [1, 1]


# ---- sparse depth from a COLMAP text model
W_, H_ = 8, 6
FOCAL = 7.0


def _colmap_scene(root):
    """4 pinhole cameras of 8 x 6 pixels on the z axis side of the origin, looking along COLMAP's +z (this project's -z) at points
    around z = 4; holdout 4 leaves views 1..3 for training.  Returns (root, poses world-to-camera [(R, t)], points, errors, tracks)."""
    from PIL import Image
    from keras_nerf_amd.data.colmap import quaternion_matrix
    model = root / "sparse" / "0"
    model.mkdir(parents=True)
    (root / "images").mkdir()
    (model / "cameras.txt").write_text(f"1 PINHOLE {W_} {H_} {FOCAL} {FOCAL} {W_ / 2} {H_ / 2}\n")
    quats = [(1.0, 0.0, 0.0, 0.0), (0.995, 0.0, 0.0998, 0.0), (0.995, 0.0998, 0.0, 0.0), (0.99, 0.05, -0.05, 0.1)]
    trans = [(0.0, 0.0, 0.0), (0.3, 0.0, 0.1), (0.0, -0.2, 0.2), (-0.2, 0.1, 0.0)]
    lines = []
    for i, (q, t) in enumerate(zip(quats, trans)):
        lines += [f"{i + 1} {' '.join(map(str, q))} {' '.join(map(str, t))} 1 v{i}.png", ""]
        Image.fromarray(np.full((H_, W_, 4), 255, np.uint8), "RGBA").save(root / "images" / f"v{i}.png")
    (model / "images.txt").write_text("\n".join(lines) + "\n")
    w2c = [(quaternion_matrix(*q), np.array(t)) for q, t in zip(quats, trans)]
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-0.8, 0.8, (10, 2)), rng.uniform(3.0, 5.0, (10, 1))], axis=1)
    # two points on one ray of view 1 (image id 2): the same pixel at two depths
    R1, t1 = w2c[1]
    ray = np.array([(5.5 - W_ / 2) / FOCAL, (2.5 - H_ / 2) / FOCAL, 1.0])
    shared = [R1.T @ (ray * s - t1) for s in (3.0, 4.5)]
    behind = np.array([0.1, 0.1, -2.0])                                    # behind every camera
    pts = np.concatenate([pts, shared, behind[None]])
    err = rng.uniform(0.2, 2.0, len(pts))
    tracks = [[1, 2, 3, 4]] * 10 + [[2], [2], [1, 2, 3, 4]]
    rows = [f"{k + 1} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} 128 128 128 {float(e)!r} " + " ".join(f"{i} 0" for i in tr) for k, (p, e, tr) in enumerate(zip(pts, err, tracks))]
    (model / "points3D.txt").write_text("# 3D point list\n" + "\n".join(rows) + "\n")
    return str(root), pts, err, tracks


def test_sparse_depth_from_a_colmap_model(tmp_path):
    from keras_nerf_amd.data.colmap import ColmapDatasetLoader
    from keras_nerf_amd.data.depth import point_weights
    from keras_nerf_amd.runtime import draw_ray_batch
    root, pts, err, tracks = _colmap_scene(tmp_path / "scene")
    ld = ColmapDatasetLoader(root, holdout=4)
    train = ld.load_dataset(1, W_, H_, 0.5, 8.0, 4)[0]
    assert len(train.image_paths) == 3
    depth, weight = ld.sparse_depth("train")
    assert depth.shape == weight.shape == (3, H_, W_) and depth.is_cuda and depth.dtype == weight.dtype == torch.float32
    depth, weight = depth.cpu().numpy(), weight.cpu().numpy()
    # the closed form in fp64, from the rays the dataset's own generator writes
    rg = train._rg_factory(0)
    c2w = torch.as_tensor(np.stack(train.camera_params))
    o = np.zeros((3, H_, W_, 3)); d = np.zeros((3, H_, W_, 3))
    for v in range(3):
        ov, dv, _ = rg(c2w[v], view_index=[v])
        o[v], d[v] = ov.cpu().numpy().astype(np.float64), dv.cpu().numpy().astype(np.float64)
    wts = point_weights(err)
    want_t, want_w = np.full((3, H_, W_), np.inf), np.zeros((3, H_, W_))
    seen_behind = 0
    for v, image_id in enumerate((2, 3, 4)):
        c2w_v = ld.poses[ld.image_ids.index(image_id)]
        for k, (p, tr) in enumerate(zip(pts, tracks)):
            if image_id not in tr:
                continue
            cam = c2w_v[:3, :3].T @ (p - c2w_v[:3, 3])                    # (right, up, backwards)
            if -cam[2] <= 0:
                seen_behind += 1
                continue
            col = int(np.floor(FOCAL * cam[0] / -cam[2] + W_ / 2)); row = int(np.floor(FOCAL * -cam[1] / -cam[2] + H_ / 2))
            if not (0 <= col < W_ and 0 <= row < H_):
                continue
            t = float(((p - o[v, row, col]) * d[v, row, col]).sum() / (d[v, row, col] ** 2).sum())
            if t < want_t[v, row, col]:
                want_t[v, row, col], want_w[v, row, col] = t, wts[k]
    hit = np.isfinite(want_t)
    assert seen_behind == 3 and 8 <= hit.sum() < 3 * H_ * W_ // 2
    assert np.array_equal(weight > 0, hit) and (depth[~hit] == 0).all()                    # empty pixels have weight 0
    rel = np.abs(depth[hit] - want_t[hit]) / want_t[hit]
    print(f"sparse depth: {hit.sum()} pixels, relative error {rel.max():.3e} / 1e-5")
    assert rel.max() <= 1e-5
    assert np.allclose(weight[hit], want_w[hit], rtol=1e-6, atol=0)
    # the shared pixel of view 0 of the split (image 2): the nearer point (s = 3) wins, with its own weight
    assert hit[0, 2, 5] and abs(want_t[0, 2, 5] - depth[0, 2, 5]) <= 1e-5 * depth[0, 2, 5] and np.isclose(weight[0, 2, 5], wts[10], rtol=1e-6)
    zn = np.linalg.norm(pts[10] - o[0, 2, 5]) / np.linalg.norm(d[0, 2, 5])
    assert abs(depth[0, 2, 5] - zn) <= 1e-3 * zn                           # the point lies on that pixel's ray, at s = 3 and not 4.5
    # batches: last_depth is the maps gathered at the draw's indices; without depth the batches are what they were
    with_depth = train.ray_batches(16, seed=4, depth=depth, depth_weight=weight)
    plain = ld.load_dataset(1, W_, H_, 0.5, 8.0, 4)[0].ray_batches(16, seed=4)
    assert plain.last_depth is None
    n = 0
    for (tp, (op, dp, t_p)), (ta, (oa, da, t_a)) in zip(plain, with_depth):
        assert torch.equal(tp, ta) and torch.equal(op, oa) and torch.equal(dp, da) and torch.equal(t_p, t_a)
        assert plain.last_depth is None
        z, c = with_depth.last_depth
        dev, cams = with_depth._resident_all()
        perm, first, cnt = with_depth.last_draw
        rgen = with_depth._rg
        index = draw_ray_batch(dev, cams, rgen.focal_length, rgen.near, rgen.far, rgen.n_sample, 4, perm, first, cnt, want_index=True,
                               camera=rgen.camera)[4].cpu().numpy()
        assert np.array_equal(z.cpu().numpy(), depth.reshape(-1)[index]) and np.array_equal(c.cpu().numpy(), weight.reshape(-1)[index])
        n += 1
    assert n == len(plain) == 3 * H_ * W_ // 16
    with_depth.set_depth(None)
    next(iter(with_depth))
    assert with_depth.last_depth is None
    only = train.ray_batches(16, seed=4, depth=depth)
    next(iter(only))
    assert only.last_depth[1] is None and only.last_depth[0].shape == (16,)
