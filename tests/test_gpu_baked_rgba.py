"""Training baked fields on RGBA on the GPU (knerf_baked_train_rays_rgba / knerf_baked_bricks_train_rays_rgba behind the background= /
opacity_loss= keywords and [n,4] targets) against tests/baked_rgba_reference.py.

Lattice, rays and seeds are those of tests/test_gpu_baked_train.py ((9, 7, 6) points, step 0.04, 150 rays, thin and opaque density) with
the one-sample rays of tests/test_gpu_baked_objective.py.  Per-ray backgrounds come from default_rng; the alphas are mixed: exact 0,
exact 1 and interior values.  Every case first asserts its preconditions on the fp64 reference alone: those of
test_gpu_baked_objective.py (clamp margins, transmittances off the threshold, opacities off the entropy clamp, a ray with one fetched
sample, one with none, rays with gaps), no difference out - tgt (tgt the target recomposited over the ray's background) within KINK of a
kink of the loss, and at least one ray each with alpha = 0, alpha = 1 and an opacity on either side of its alpha.

Bound per tensor and per term: max(1e-5 x max |fp64|, 4 x the deviation of the float32 run of the reference over 8 ray orders, in both
summation orders where a term of the weights has a gradient).  Measured on the CPU, never on the kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import baked_objective_reference as Q
from tests import baked_rgba_reference as P
from tests import baked_train_reference as T
from tests import test_gpu_baked_objective as O
from tests import test_gpu_baked_train as B

pytestmark = pytest.mark.gpu

RES, LO, HI, STEP, N_RAYS = B.RES, B.LO, B.HI, B.STEP, B.N_RAYS
THIN, OPAQUE, TERMINATION, MARGIN, KINK = B.THIN, B.OPAQUE, B.TERMINATION, B.MARGIN, O.KINK
DIST, ENT, OPA = 0.5, 0.05, 0.3
# name: (reference keywords, alpha targets, optimiser keywords)
OBJECTIVES = {"mse+opacity": (dict(loss_kind=Q.MSE, opacity=OPA), True),
              "huber+reg+opacity": (dict(loss_kind=Q.HUBER, huber_delta=0.05, distortion=DIST, opacity_entropy=ENT, opacity=OPA), True),
              "mae+background": (dict(loss_kind=Q.MAE), False)}
NAMES = tuple(OBJECTIVES)
ENVS = ((THIN, 0.0), (OPAQUE, 0.0), (OPAQUE, TERMINATION))


def _keywords(name):
    from keras_nerf_amd import losses
    return {"mse+opacity": dict(opacity_loss=OPA),
            "huber+reg+opacity": dict(loss=losses.Huber(0.05), regularizers=losses.RayRegularizers(distortion=DIST, opacity_entropy=ENT),
                                      opacity_loss=OPA),
            "mae+background": dict(loss="mae")}[name]


def _backgrounds(seed=7):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (N_RAYS, 3)).astype(np.float32)


def _alphas(seed=8):
    """interior values with every third ray exactly 0 and every fifth (from 1) exactly 1"""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.05, 0.95, N_RAYS).astype(np.float32)
    alpha[::3] = 0.0
    alpha[1::5] = 1.0
    return alpha


_cases = {}


def _case(degree, dense, termination, name, stored, mode="mixed"):
    """lattice, rays, backgrounds, alphas, the fp64 reference with its preconditions checked, and the bounds: computed once per case.
    mode "own": alpha = 1 rays keep their random background, every other ray has the stored background, so that tgt is the target
    itself, and the target is the reference's own output: every d is exactly 0 and only the opacity term has a gradient"""
    key = (degree, dense, termination, name, stored, mode)
    if key in _cases:
        return _cases[key]
    sigma, co = B._lattice(degree, dense)
    rays = O._rays(degree)
    support = T.support_cells(sigma)
    obj, with_alpha = OBJECTIVES[name]
    bg, alpha = _backgrounds(), (_alphas() if with_alpha else None)
    geo = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP)
    target = rays["target"]
    if mode == "own":
        bg[alpha != 1.0] = np.float32(stored)
        probe = {}
        P.loss_and_grad(*geo, target, support, background=bg, termination=termination, info=probe)
        target = probe["out"]                                              # float64: the reference's d is exactly 0
    kw = dict(background=bg, alpha=alpha, stored=stored, termination=termination, **obj)
    args = geo + (target, support)
    info = {}
    L, terms, gs, gc = P.loss_and_grad(*args, **kw, info=info)
    raw, pre, opa, Tn, kept = info["raw"], info["pre"], info["opacity"], info["T"], info["kept"]
    hit = opa > 0
    assert min(np.abs(raw).min(), np.abs(raw - 1).min()) >= MARGIN, (key, "a raw colour on a clamp edge")
    assert min(np.abs(pre[hit]).min(), np.abs(pre[hit] - 1).min()) >= MARGIN, (key, "an output on a clamp edge")
    assert (pre[~hit] == bg[~hit]).all()
    if termination:
        assert (Tn < termination).sum() >= 20 and np.abs(Tn / termination - 1).min() >= 1e-3, (key, "a transmittance on the threshold")
    d = np.abs(info["out"] - info["tgt"])                                 # every ray: tgt is formed in float32 by the kernel
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
    names = ("gs", "gc", "L") + P.TERMS
    dev = {k: 0.0 for k in names}
    rng = np.random.default_rng(99)
    weights = obj.get("distortion", 0) > 0 or obj.get("opacity_entropy", 0) > 0 or obj.get("opacity", 0) > 0
    for _ in range(8):                                                     # the fp32 reference's own error over 8 accumulation orders
        order = rng.permutation(N_RAYS)
        for mirror in ((False, True) if weights else (False,)):
            L32, t32, s32, c32 = P.loss_and_grad(*args, **kw, dtype=np.float32, order=order, mirror=mirror)
            dev["gs"], dev["gc"] = max(dev["gs"], float(np.abs(s32 - gs).max())), max(dev["gc"], float(np.abs(c32 - gc).max()))
            dev["L"] = max(dev["L"], abs(L32 - L))
            for k in P.TERMS:
                dev[k] = max(dev[k], abs(t32[k] - terms[k]))
    ref = {"gs": gs, "gc": gc, "L": L, **terms}
    bound = {k: max(1e-5 * float(np.abs(ref[k]).max()), 4.0 * dev[k]) for k in dev}
    _cases[key] = {"sigma": sigma, "co": co, "rays": rays, "target": target, "support": support, "bg": bg, "alpha": alpha, "stored": stored,
                   "ref": ref, "bound": bound, "dev": dev, "info": info}
    return _cases[key]


def _field(case):
    from keras_nerf_amd.baked import BakedField
    return BakedField.from_arrays(case["sigma"], case["co"], (LO, HI))


def _target(case, sl=slice(None)):
    """the float32 target of the case, [n,4] with its alphas where it has them"""
    tg = np.asarray(case["target"], dtype=np.float32)[sl]
    return tg if case["alpha"] is None else np.concatenate([tg, case["alpha"][sl, None]], axis=1)


def _batch(case, sl=slice(None)):
    r = case["rays"]
    return r["o"][sl], r["d"][sl], r["near"][sl], r["far"][sl], _target(case, sl)


def _compare(opt, loss, case, what):
    """gradient, loss and the five terms of an accumulate() against the case's fp64 reference, each within its bound"""
    ref, bound = case["ref"], case["bound"]
    gs, gc = (g.cpu().numpy() for g in opt.gradients())
    got = {"gs": gs, "gc": gc, "L": float(loss), **{k: float(v) for k, v in opt.objective_terms().items()}}
    assert loss.dtype == torch.float64 and loss.dim() == 0 and tuple(opt.objective_terms()) == P.TERMS
    slots = T.slot_points(case["support"])
    assert (gs[~slots] == 0).all() and (gc[~slots] == 0).all()
    line = []
    for k in bound:
        err = float(np.abs(got[k] - ref[k]).max())
        line.append(f"{k} {err:.3e} / {bound[k]:.3e} (fp32 {case['dev'][k]:.3e}, max {float(np.abs(ref[k]).max()):.3e})")
        assert err <= bound[k], (what, k, err, bound[k])
    print(f"{what}: error / bound  " + "; ".join(line))


def _target_background(stored):
    return "white" if stored else "black"


# every (degree, objective) pair; the three environments dealt out so that every degree and every objective sees each of them
GRADIENT_CASES = [(deg, *ENVS[(deg + k) % 3], NAMES[k], float((deg + k) % 2)) for deg in range(4) for k in range(3)]


@pytest.mark.parametrize("degree,dense,termination,name,stored", GRADIENT_CASES)
def test_gradient_and_terms_match_fp64(degree, dense, termination, name, stored):
    """dense and bricks, every lane variant; the background is the per-call tensor"""
    from keras_nerf_amd.baked_bricks_train import BRICK_TRAIN_VARIANTS
    from keras_nerf_amd.baked_train import brick_optimizer
    case = _case(degree, dense, termination, name, stored)
    kw = dict(step=STEP, termination=termination, target_background=_target_background(stored), **_keywords(name))
    what = f"degree {degree} dense {dense} termination {termination} {name} stored {stored}"
    for lanes in B.VARIANTS[degree]:
        opt = _field(case).optimizer(0.05, 0.01, lanes_per_ray=lanes, **kw)
        assert opt.objective_terms() is None and opt.last_background is None
        loss = opt.accumulate(*_batch(case), background=case["bg"])
        assert np.array_equal(opt.last_background.cpu().numpy(), case["bg"])
        _compare(opt, loss, case, f"{what} lanes {lanes}")
    bricks = _field(case).compact(4)
    for lanes in (0,) + BRICK_TRAIN_VARIANTS[degree]:
        opt = brick_optimizer(bricks, 0.05, 0.01, lanes_per_ray=lanes, **kw)
        loss = opt.accumulate(*_batch(case), background=case["bg"])
        _compare(opt, loss, case, f"{what} bricks lanes {lanes}")


def _one_ray_at_a_time(opt, case, target=None, background=None, collect=None):
    o, d, near, far, tg = _batch(case)
    tg = tg if target is None else target
    for r in range(N_RAYS):
        extra = {} if background is None else dict(background=background[r:r + 1])
        loss = opt.accumulate(o[r:r + 1], d[r:r + 1], near[r:r + 1], far[r:r + 1], tg[r:r + 1], n_total=N_RAYS, **extra)
        if collect is not None:
            collect.append((loss, opt.objective_terms()))


def _same(seen_a, seen_b, names):
    for (la, ta), (lb, tb) in zip(seen_a, seen_b):
        assert torch.equal(la, lb) and all(torch.equal(ta[k], tb[k]) for k in names)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_flag_anchors_bit_for_bit(degree):
    """a background of ones (zeros) without alpha and weight is the white (black) flag's _ext launch; one ray per launch fixes the order
    of the atomic adds"""
    case = _case(degree, THIN, 0.0, "huber+reg+opacity", 0.0)
    rgb = np.asarray(case["target"], dtype=np.float32)
    kw = _keywords("huber+reg+opacity")
    del kw["opacity_loss"]
    for white in (False, True):
        full = np.full((N_RAYS, 3), 1.0 if white else 0.0, dtype=np.float32)
        for lanes in B.VARIANTS[degree]:
            ext = _field(case).optimizer(0.05, 0.01, step=STEP, white_background=white, lanes_per_ray=lanes, **kw)
            rgba = _field(case).optimizer(0.05, 0.01, step=STEP, lanes_per_ray=lanes, **kw)
            seen_e, seen_r = [], []
            _one_ray_at_a_time(ext, case, target=rgb, collect=seen_e)
            _one_ray_at_a_time(rgba, case, target=rgb, background=full, collect=seen_r)
            assert tuple(seen_e[0][1]) == Q.TERMS and tuple(seen_r[0][1]) == P.TERMS
            _same(seen_e, seen_r, ("photometric", "mse", "distortion", "opacity_entropy"))
            assert torch.equal(ext._grad, rgba._grad) and float(ext._grad.abs().max()) > 0, (degree, white, lanes)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_alpha_one_is_no_alpha_bit_for_bit(degree):
    """alpha = 1 everywhere with weight 0: the bits of the same call without alpha"""
    case = _case(degree, THIN, 0.0, "huber+reg+opacity", 1.0)
    rgb = np.asarray(case["target"], dtype=np.float32)
    rgba1 = np.concatenate([rgb, np.ones((N_RAYS, 1), np.float32)], axis=1)
    kw = _keywords("huber+reg+opacity")
    del kw["opacity_loss"]
    for lanes in B.VARIANTS[degree]:
        a = _field(case).optimizer(0.05, 0.01, step=STEP, lanes_per_ray=lanes, target_background="white", **kw)
        b = _field(case).optimizer(0.05, 0.01, step=STEP, lanes_per_ray=lanes, target_background="white", **kw)
        seen_a, seen_b = [], []
        _one_ray_at_a_time(a, case, target=rgb, background=case["bg"], collect=seen_a)
        _one_ray_at_a_time(b, case, target=rgba1, background=case["bg"], collect=seen_b)
        _same(seen_a, seen_b, ("photometric", "mse", "distortion", "opacity_entropy"))
        assert torch.equal(a._grad, b._grad) and float(a._grad.abs().max()) > 0, (degree, lanes)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("b", [4, 8])
def test_bricks_equal_dense(degree, b):
    """under the full rgba objective, bit for bit"""
    from keras_nerf_amd.baked_bricks_train import BRICK_TRAIN_VARIANTS
    from keras_nerf_amd.baked_train import brick_optimizer
    stored = float(degree % 2)
    case = _case(degree, THIN, 0.0, "huber+reg+opacity", stored)
    bricks = _field(case).compact(b)
    dense = bricks.to_dense()
    for lanes in (0,) + BRICK_TRAIN_VARIANTS[degree]:
        kw = dict(step=STEP, lanes_per_ray=lanes, target_background=_target_background(stored), **_keywords("huber+reg+opacity"))
        D, S = dense.optimizer(0.05, 0.01, **kw), brick_optimizer(bricks, 0.05, 0.01, **kw)
        seen_d, seen_s = [], []
        _one_ray_at_a_time(D, case, background=case["bg"], collect=seen_d)
        _one_ray_at_a_time(S, case, background=case["bg"], collect=seen_s)
        _same(seen_d, seen_s, P.TERMS)
        for gd, gs in zip(D.gradients(), S.gradients()):
            assert torch.equal(gd, gs) and float(gd.abs().max()) > 0


@pytest.mark.parametrize("degree,dense,termination,stored", [(0, OPAQUE, 0.0, 0.0), (1, THIN, 0.0, 1.0), (2, OPAQUE, TERMINATION, 1.0),
                                                             (3, THIN, 0.0, 0.0)])
def test_opacity_only_gradient(degree, dense, termination, stored):
    """the target is the field's own image over the rays' backgrounds, rendered by the march the optimiser uses, and tgt is the target
    itself (alpha = 1, or the stored background): every d is exactly 0, g is 0 on every channel and the gradient is the opacity term's
    alone -- a kernel that leaves at `g == 0` without looking at the opacity weight adds nothing"""
    case = _case(degree, dense, termination, "mse+opacity", stored, mode="own")
    assert float(np.abs(case["ref"]["gs"]).max()) > 1e-7 and float(np.abs(case["ref"]["gc"]).max()) == 0.0
    rays, bg = case["rays"], torch.as_tensor(case["bg"])
    for lanes in B.VARIANTS[degree]:
        opt = _field(case).optimizer(0.05, 0.01, step=STEP, termination=termination, lanes_per_ray=lanes,
                                     target_background=_target_background(stored), opacity_loss=OPA)
        img = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, termination=termination, lanes_per_ray=lanes,
                               outputs="image", background=bg)["image"]
        target = torch.cat([img, torch.as_tensor(case["alpha"]).to(img.device)[:, None]], dim=1)
        loss = opt.accumulate(rays["o"], rays["d"], rays["near"], rays["far"], target, background=bg)
        terms = opt.objective_terms()
        assert float(terms["photometric"]) == 0.0 and float(terms["mse"]) == 0.0 and float(terms["opacity"]) > 0.0
        assert float(opt._grad[:, 1:].abs().max()) == 0.0 and float(opt._grad[:, 0].abs().max()) > 0.0
        _compare(opt, loss, case, f"opacity only: degree {degree} dense {dense} termination {termination} lanes {lanes}")


_floater = {}


def _floater_case(degree):
    """records whose colour evaluates to exactly 0 (every coefficient 0) in front of rays with a black target and alpha = 0"""
    if degree in _floater:
        return _floater[degree]
    sigma, co = B._lattice(degree, THIN)
    co = np.zeros_like(co)
    rays = O._rays(degree)
    support = T.support_cells(sigma)
    bg = np.random.default_rng(21).uniform(0.2, 0.9, (N_RAYS, 3)).astype(np.float32)
    geo = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP, np.zeros((N_RAYS, 3), np.float32), support)
    kw = dict(background=bg, alpha=np.zeros(N_RAYS, np.float32), stored=0.0)
    info = {}
    L, terms, gs, gc = P.loss_and_grad(*geo, **kw, info=info)
    hit = info["opacity"] > 0
    assert (info["raw"] == 0).all() and hit.sum() >= 90
    assert min(np.abs(info["pre"][hit]).min(), np.abs(info["pre"][hit] - 1).min()) >= MARGIN
    black = P.loss_and_grad(*geo, background=None, alpha=kw["alpha"], stored=0.0)
    assert black[0] == 0.0 and (black[2] == 0).all() and (black[3] == 0).all()      # invisible: the gradient is exactly zero
    dev = {"gs": 0.0, "gc": 0.0}
    rng = np.random.default_rng(99)
    for _ in range(8):
        _, _, s32, c32 = P.loss_and_grad(*geo, **kw, dtype=np.float32, order=rng.permutation(N_RAYS))
        dev["gs"], dev["gc"] = max(dev["gs"], float(np.abs(s32 - gs).max())), max(dev["gc"], float(np.abs(c32 - gc).max()))
    bound = {"gs": max(1e-5 * float(np.abs(gs).max()), 4.0 * dev["gs"]), "gc": max(1e-5 * float(np.abs(gc).max()), 4.0 * dev["gc"])}
    _floater[degree] = {"sigma": sigma, "co": co, "rays": rays, "bg": bg, "gs": gs, "gc": gc, "bound": bound, "support": support}
    return _floater[degree]


@pytest.mark.parametrize("degree", [0, 2])
def test_the_invisible_floater(degree):
    """density whose colour is exactly black in front of empty black pixels: under the black background prediction and target agree and
    the gradient is exactly 0 everywhere; over a per-ray background the floater hides the background the photograph shows, and the
    gradient of sigma at every trainable point a ray weighs is > 0 (less density lowers the loss) and matches fp64"""
    case = _floater_case(degree)
    rays = case["rays"]
    rgb, rgba = np.zeros((N_RAYS, 3), np.float32), np.zeros((N_RAYS, 4), np.float32)
    batch = (rays["o"], rays["d"], rays["near"], rays["far"])
    trainable = T.sigma_trainable(case["support"])
    for lanes in B.VARIANTS[degree]:
        for kw, target in ((dict(), rgb), (dict(background="black"), rgb), (dict(background="black"), rgba)):
            opt = _field(case).optimizer(0.05, 0.01, step=STEP, lanes_per_ray=lanes, **kw)
            loss = opt.accumulate(*batch, target)
            assert float(loss) == 0.0 and float(opt._grad.abs().max()) == 0.0, (lanes, kw)
        opt = _field(case).optimizer(0.05, 0.01, step=STEP, lanes_per_ray=lanes)
        loss = opt.accumulate(*batch, rgba, background=case["bg"])
        gs, gc = (g.cpu().numpy() for g in opt.gradients())
        assert float(loss) > 1e-3
        weighed = case["gs"] != 0
        assert weighed.sum() > 50 and (case["gs"][weighed] > 0).all() and (gs[weighed] > 0).all()
        for k, got in (("gs", gs), ("gc", gc)):
            err = float(np.abs(got - case[k]).max())
            print(f"floater degree {degree} lanes {lanes}: {k} error {err:.3e} / bound {case['bound'][k]:.3e}")
            assert err <= case["bound"][k], (k, err, case["bound"][k])
        assert (gs[~T.slot_points(case["support"])] == 0).all() and trainable.any()


# final / initial objective (2.9540e-03 -> 2.2056e-05) of P.optimise on the same 40 steps (mse, opacity_loss 0.01, the backgrounds of
# _random_backgrounds, the first of them again for the final value), float64 on the CPU
REFERENCE_RATIO = 7.467e-3
OPT_OPACITY = 0.01


def _random_backgrounds():
    rng = np.random.default_rng(40)
    return [rng.uniform(0.0, 1.0, (N_RAYS, 3)).astype(np.float32) for _ in range(40)]


def _optimise_setup():
    """tests/test_gpu_baked_train.py's optimisation with field A's own opacity as the alpha of its image (over black)"""
    from tests import baked_reference as R
    sigma, co = B._lattice(2, THIN)
    sigma0, co0, rays, target = B._optimise_setup()
    alpha = R.march(sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP)[2].astype(np.float32)
    return sigma0, co0, rays, target, alpha


def test_it_optimises(monkeypatch):
    """40 steps with background="random" and an opacity loss, through BakedFieldOptimizer and through grid_trainer: the GPU reaches at
    most twice the float64 NumPy optimiser's final / initial objective (the margin of tests/test_gpu_baked_train.py).  torch.rand is
    replaced by the tensors of _random_backgrounds, so that the reference ran under the same backgrounds."""
    from keras_nerf_amd.baked import BakedField
    from keras_nerf_amd.baked_bricks_grow import grid_trainer
    sigma, co, rays, target, alpha = _optimise_setup()
    start = BakedField.from_arrays(sigma, co, (LO, HI))
    target4 = torch.as_tensor(np.concatenate([target, alpha[:, None]], axis=1))
    batches = [(target4, (rays["o"], rays["d"], None))] * 40
    backgrounds = _random_backgrounds()
    for build in (lambda **kw: start.optimizer(*B.OPT_RATES, step=STEP, **kw), lambda **kw: grid_trainer(start.compact(4), *B.OPT_RATES, step=STEP, **kw)):
        opt = build(background="random", opacity_loss=OPT_OPACITY, background_seed=3)
        queue = list(backgrounds)

        def rand(shape, device=None, dtype=None, generator=None):
            assert tuple(shape) == (N_RAYS, 3) and generator is not None and dtype == torch.float32
            return torch.as_tensor(queue.pop(0)).to(device)
        monkeypatch.setattr(torch, "rand", rand)
        hist = opt.fit(batches, rays["near"], rays["far"])
        monkeypatch.undo()
        assert not queue and np.array_equal(opt.last_background.cpu().numpy(), backgrounds[-1])
        final = float(opt.accumulate(rays["o"], rays["d"], rays["near"], rays["far"], target4, background=backgrounds[0]))
        assert len(hist["loss"]) == 40 and all(len(hist[k]) == 40 for k in P.TERMS)
        assert abs(hist["loss"][3] - (hist["photometric"][3] + float(np.float32(OPT_OPACITY)) * hist["opacity"][3])) <= 1e-15
        ratio = final / hist["loss"][0]
        print(f"{type(opt).__name__}: objective {hist['loss'][0]:.4e} -> {final:.4e}: ratio {ratio:.4e} (reference {REFERENCE_RATIO})")
        assert ratio <= 2.0 * REFERENCE_RATIO


def test_random_backgrounds_come_from_one_seeded_device_generator():
    case = _case(0, THIN, 0.0, "mse+opacity", 0.0)
    draws = []
    for seed in (5, 5, 6):
        opt = _field(case).optimizer(0.05, 0.01, step=STEP, background="random", background_seed=seed)
        got = []
        for _ in range(2):
            opt.accumulate(*_batch(case))
            bg = opt.last_background
            assert bg.is_cuda and bg.shape == (N_RAYS, 3) and bg.dtype == torch.float32 and float(bg.min()) >= 0.0 and float(bg.max()) < 1.0
            got.append(bg.clone())
        assert not torch.equal(got[0], got[1])                             # the generator goes on: a new background per launch
        draws.append(got)
    assert all(torch.equal(a, b) for a, b in zip(draws[0], draws[1])) and not torch.equal(draws[0][0], draws[2][0])
    with pytest.raises(ValueError):
        _field(case).optimizer(0.05, 0.01, step=STEP, background="random").accumulate(*_batch(case)[:4], np.zeros((N_RAYS, 3), np.float32))


class _Counting:
    """the library with every call of a knerf_baked_*train_rays* function counted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if "train_rays" not in name:
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def test_white_keyword_is_the_white_flag_and_no_keyword_is_the_old_call(monkeypatch):
    from keras_nerf_amd import _lib, losses
    from keras_nerf_amd.baked_train import brick_optimizer
    case = _case(2, THIN, 0.0, "mae+background", 0.0)
    counting = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: counting)
    rgb = np.asarray(case["target"], dtype=np.float32)
    for objective, suffix in ((dict(), ""), (dict(loss=losses.Huber(0.05)), "_ext")):
        for build, name in ((lambda **kw: _field(case).optimizer(0.05, 0.01, step=STEP, **kw), "knerf_baked_train_rays"),
                            (lambda **kw: brick_optimizer(_field(case).compact(4), 0.05, 0.01, step=STEP, **kw), "knerf_baked_bricks_train_rays")):
            a, b = build(white_background=True, **objective), build(background="white", **objective)
            assert b.white_background is True
            for _ in range(2):
                counting.calls.clear()
                la, lb = [], []
                _one_ray_at_a_time(a, case, target=rgb, collect=la)
                _one_ray_at_a_time(b, case, target=rgb, collect=lb)
                assert counting.calls == [name + suffix] * (2 * N_RAYS)            # the entry points of an optimiser without the keywords
                assert all(torch.equal(x[0], y[0]) for x, y in zip(la, lb)) and torch.equal(a._grad, b._grad)
                a.apply(); b.apply()
                for x, y in ((a.field._records, b.field._records), (a._master, b._master), (a._m, b._m), (a._v, b._v)):
                    assert torch.equal(x, y)
            counting.calls.clear()
            build(**objective).accumulate(*_batch(case)[:4], rgb)
            build(background="black", target_background="white", background_seed=9, **objective).accumulate(*_batch(case)[:4], rgb)
            assert counting.calls == [name + suffix] * 2
    with pytest.raises(ValueError):
        _field(case).optimizer(0.05, 0.01, white_background=True, background="black")


def test_rgba_entry_points_refuse_bad_arguments_before_any_launch():
    """on live optimisers with valid device pointers: every bad record is refused and the gradient buffer stays zero"""
    from keras_nerf_amd import _lib
    from keras_nerf_amd.baked import _stream
    from keras_nerf_amd.baked_train import brick_optimizer
    from keras_nerf_amd.runtime import _f32, _ptr
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    case = _case(2, THIN, 0.0, "huber+reg+opacity", 0.0)
    o, d, near, far, tg = (_f32(x, "cuda") for x in _batch(case))
    rgb, alpha, bg = tg[:, :3].contiguous(), tg[:, 3].contiguous(), _f32(case["bg"], "cuda")
    terms = torch.zeros((N_RAYS, 5), device="cuda")
    sq = torch.zeros((N_RAYS,), device="cuda")
    huber = _lib.KnerfObjective(_lib.LOSS_HUBER, 0.1, 0.01, 1e-3, 3)
    for opt, fn in ((_field(case).optimizer(0.05, 0.01, step=STEP), lib.knerf_baked_train_rays_rgba),
                    (brick_optimizer(_field(case).compact(4), 0.05, 0.01, step=STEP), lib.knerf_baked_bricks_train_rays_rgba)):
        flags = _lib.BAKED_SKIP_EMPTY
        terms.zero_()

        def call(rec, ob=None, step=STEP, fl=flags, target=rgb):
            return fn(_stream(o.device), C.byref(opt._c), _ptr(o), _ptr(d), _ptr(near), _ptr(far), 0.0, 0.0, _ptr(target), N_RAYS, 0, step, 0.0,
                      fl, _ptr(sq), C.byref(ob) if ob is not None else None, _ptr(terms), C.byref(rec))
        P_, A_ = bg.data_ptr(), alpha.data_ptr()
        for bad in ((P_, A_, 0.5, 0.1), (P_, A_, -1.0, 0.1), (P_, A_, float("nan"), 0.1), (P_, A_, 0.0, -0.1), (P_, A_, 0.0, float("nan")),
                    (P_, A_, 0.0, float("inf")), (P_, None, 0.0, 0.1), (None, None, 1.0, 1e-3), (None, None, 2.0, 0.0)):
            for ob in (None, huber):
                assert call(_lib.KnerfBakedRgba(*bad), ob) == INV, bad
        good = _lib.KnerfBakedRgba(P_, A_, 0.0, 0.1)
        assert call(good, _lib.KnerfObjective(7, 0.1, 0.0, 0.0, 3)) == INV and call(good, _lib.KnerfObjective(_lib.LOSS_MSE, 0.0, -1.0, 0.0, 3)) == INV
        assert call(good, step=0.0) == INV and call(good, fl=4) == INV and call(good, fl=2 << 8) == INV and call(good, target=None) == INV
        torch.cuda.synchronize()
        assert float(opt._grad.abs().max()) == 0.0 and float(terms.abs().max()) == 0.0
        assert call(good, huber) == 0
        torch.cuda.synchronize()
        assert float(opt._grad.abs().max()) > 0.0 and float(terms[:, 4].max()) > 0.0
    with pytest.raises(ValueError, match="QuantizedBrickField"):
        brick_optimizer(_field(case).compact(4).quantize(), 0.05, 0.01, background="random")


def test_ray_batches_with_alpha(tmp_path):
    """3 views of 8 x 8: o, d, t and rgb are those of alpha=False at the same seed, the fourth column is the images' alpha"""
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.runtime import draw_ray_batch
    from tests.synthetic_scene import write
    root = write(str(tmp_path / "scene"), n=(3, 1, 1))
    load = lambda: DatasetLoader(root, white_background=True).load_dataset(1, 8, 8, 2.0, 6.0, 16)[0]
    plain, rgba = load().ray_batches(64, seed=4), load().ray_batches(64, seed=4, alpha=True)
    assert len(plain) == len(rgba) == 3 and rgba.alpha and not plain.alpha
    seen = []
    for (tp, (op, dp, t_p)), (ta, (oa, da, t_a)) in zip(plain, rgba):
        assert tp.shape == (64, 3) and ta.shape == (64, 4) and ta.is_cuda and ta.dtype == torch.float32
        assert torch.equal(op, oa) and torch.equal(dp, da) and torch.equal(t_p, t_a) and torch.equal(tp, ta[:, :3])
        dev, cams = rgba._resident_all()
        perm, first, n = rgba.last_draw
        index = draw_ray_batch(dev, cams, rgba._rg.focal_length, 2.0, 6.0, 16, 4, perm, first, n, want_index=True)[4]
        assert torch.equal(ta[:, 3], dev.reshape(-1, 4)[index, 3])
        seen.append(ta[:, 3].cpu().numpy())
    seen = np.concatenate(seen)
    assert (seen == 0).any() and (seen == 1).any()                         # the cut-outs' empty and covered pixels


@pytest.mark.parametrize("kind", ["dense", "bricks", "quantized"])
def test_render_over_a_background(kind):
    """(1, 1, 1) is within 2 ulp of 1.0 per channel of white_background=True (two float32 roundings against one); a zero background is
    the black render exactly; an [n,3] tensor is the composition of the black launch"""
    case = _case(2, THIN, 0.0, "mae+background", 0.0)
    field = _field(case)
    field = {"dense": lambda: field, "bricks": lambda: field.compact(4), "quantized": lambda: field.compact(4).quantize()}[kind]()
    rays = case["rays"]
    args = (rays["o"], rays["d"], rays["near"], rays["far"])
    black = field.render(*args, step=STEP)
    white = field.render(*args, step=STEP, white_background=True)
    over1 = field.render(*args, step=STEP, background=(1, 1, 1))
    over0 = field.render(*args, step=STEP, background=(0.0, 0.0, 0.0))
    assert sorted(over1) == sorted(black) == ["depth", "image", "opacity"]
    ulp = float(np.spacing(np.float32(1.0)))
    assert float((over1["image"] - white["image"]).abs().max()) <= 2 * ulp and not torch.equal(white["image"], black["image"])
    for k in ("image", "depth", "opacity"):
        assert torch.equal(over0[k], black[k]) and (k == "image" or torch.equal(over1[k], black[k]))
    bg = torch.as_tensor(case["bg"]).cuda()
    got = field.render(*args, step=STEP, background=bg, outputs="image")
    assert sorted(got) == ["image"]
    assert torch.equal(got["image"], (black["image"] + (1.0 - black["opacity"])[:, None] * bg).clamp(0.0, 1.0))
    for bad in (dict(background=(1, 1, 1), white_background=True), dict(background=(1, 1)), dict(background=bg[:5]), dict(background=bg * 2)):
        with pytest.raises(ValueError):
            field.render(*args, step=STEP, **bad)
