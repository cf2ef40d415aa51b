"""Growing a baked field on the GPU (keras_nerf_amd/baked.py, baked_train.py, csrc/baked_grow.hip) against
tests/baked_grow_reference.py: the TV gradient and value for every SH degree, the one deterministic add, resampling byte for byte, the
regularised step, the support invariant with TV on, a coarse-to-fine fit, and the refusals.

Lattice (9, 7, 6) with two empty interior cells and two empty cell layers, and the ray set: those of tests/test_gpu_baked_train.py,
rebuilt here (same seeds, so the preconditions chosen there hold: no raw colour, output or transmittance on a kink).
Tolerances and measured values: tests/README_baked_grow.md.  No element is left out of any comparison.

Coarse to fine (test_coarse_to_fine): the NumPy loop (tests/baked_grow_reference.py fit_coarse_to_fine, float64, run inside the test)
brings the loss from 2.1668e-3 to 6.0935e-6 over [(None, 20), ((17, 13, 11), 20)] (ratio 2.812e-3); the GPU: see the README."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import baked_grow_reference as G
from tests import baked_reference as R
from tests import baked_train_reference as T

pytestmark = pytest.mark.gpu

RES, FINE = (9, 7, 6), (17, 13, 11)
LO, HI = (-1.0, -0.8, -0.6), (1.0, 0.8, 0.7)
STEP = 0.04
N_RAYS = 150
MARGIN = 1e-4
THIN = 0.1
SEEDS = {0: 1, 1: 1, 2: 1, 3: 2}
COEF_SCALE = {0: 0.6, 1: 0.6, 2: 0.4, 3: 0.3}
TV = dict(tv_sigma=2e-2, tv_sh=5e-2, tv_epsilon=1e-6)
U = 2.0 ** -24


def _lattice(degree, dense=THIN):
    rng = np.random.default_rng(300 + SEEDS[degree])
    sigma = rng.uniform(0.0, 30.0, RES).astype(np.float32) * np.float32(dense)
    sigma[0], sigma[-1], sigma[:, 0], sigma[:, -1], sigma[:, :, 0], sigma[:, :, -1] = 0, 0, 0, 0, 0, 0     # no jump at the box face
    sigma[3:6, 2:4, 2:4] = 0                                                                              # two empty interior cells
    sigma[6:] = 0                                                                                         # and two empty layers of cells
    K = (degree + 1) ** 2
    co = (rng.standard_normal(RES + (K, 3)) * COEF_SCALE[degree]).astype(np.float16)
    co[..., 0, :] += np.float16(1.5)
    return sigma, co


def _rays(degree):
    """150 rays: 0..89 cross the box from outside, 90..109 miss it, 110..129 start inside, 130..141 have one or two direction components
    exactly 0, 142..149 have directions that are no unit vectors; and one target colour per ray"""
    rng = np.random.default_rng(17 + 1000 * SEEDS[degree])
    lo, hi = np.array(LO), np.array(HI)
    mid = 0.5 * (lo + hi)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    o = mid + 3.0 * unit(rng.standard_normal((N_RAYS, 3)))
    aim = rng.uniform(lo + 0.1, hi - 0.1, (N_RAYS, 3))
    aim[:, 0] = rng.uniform(-0.9, 0.2, N_RAYS)
    d = unit(aim - o)
    near, far = rng.uniform(0.0, 0.5, N_RAYS), rng.uniform(5.0, 6.5, N_RAYS)
    d[90:110] = unit(o[90:110] - mid + 0.3 * rng.standard_normal((20, 3)))
    o[110:130] = rng.uniform(lo + 0.05, hi - 0.05, (20, 3)); d[110:130] = unit(rng.standard_normal((20, 3))); near[110:130] = 0.0
    for i in range(130, 138):
        a = i % 3
        t = rng.uniform(lo + 0.2, hi - 0.2)
        o[i][a] = t[a]
        d[i] = t - o[i]; d[i][a] = 0.0; d[i] = unit(d[i])
    for i in range(138, 142):
        a = i % 3
        o[i] = rng.uniform(lo + 0.2, hi - 0.2); d[i] = 0.0; d[i][a] = 1.0 if i % 2 else -1.0
        o[i][a] = mid[a] - 3.0 * d[i][a]
    for i, s in zip(range(142, 150), (2.5, 0.3, 7.0, 1.0 / 3.0, 1.7, 0.6, 4.0, 0.45)):
        d[i] *= s; near[i] /= s; far[i] /= s
    target = rng.uniform(0.0, 1.0, (N_RAYS, 3))
    return {"o": o.astype(np.float32), "d": d.astype(np.float32), "near": near.astype(np.float32), "far": far.astype(np.float32),
            "target": target.astype(np.float32)}


def _field(sigma, co, bounds=(LO, HI)):
    from keras_nerf_amd.baked import BakedField
    return BakedField.from_arrays(sigma, co, bounds)


def _batch(rays):
    return rays["o"], rays["d"], rays["near"], rays["far"], rays["target"]


_ray_case = {}


def _case():
    """degree 2, thin, black background: the fp64 loss and gradient, their preconditions, and the bound of the section 2.20 gradient test
    (max(1e-5 max |g|, 4 x the fp32 reference's deviation over 8 ray orders)); computed once and shared"""
    if _ray_case:
        return _ray_case
    sigma, co = _lattice(2)
    rays = _rays(2)
    support = T.support_cells(sigma)
    args = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP, rays["target"], support, False, 0.0)
    info = {}
    L, gs, gc, _ = T.loss_and_grad(*args, info=info)
    raw, pre, opa = info["raw"], info["pre"], info["opacity"]
    hit = opa > 0
    assert min(np.abs(raw).min(), np.abs(raw - 1).min()) >= MARGIN and min(np.abs(pre[hit]).min(), np.abs(pre[hit] - 1).min()) >= MARGIN
    dev_s = dev_c = 0.0
    rng = np.random.default_rng(99)
    for _ in range(8):
        _, s32, c32, _ = T.loss_and_grad(*args, dtype=np.float32, order=rng.permutation(N_RAYS))
        dev_s, dev_c = max(dev_s, float(np.abs(s32 - gs).max())), max(dev_c, float(np.abs(c32 - gc).max()))
    _ray_case.update(sigma=sigma, co=co, rays=rays, support=support, L=L, gs=gs, gc=gc,
                     bound=(max(1e-5 * float(np.abs(gs).max()), 4.0 * dev_s), max(1e-5 * float(np.abs(gc).max()), 4.0 * dev_c)))
    return _ray_case


def _tv_setup(degree, **tv):
    """an optimiser on the lattice whose master rows are perturbed by noise (the sigma of a non-trainable slot stays 0) and hold a block
    of equal rows; (optimiser, master fp64 [n_slots, W], slot_of, has [RES], trainable [RES])"""
    sigma, co = _lattice(degree)
    sigma[2:5, 2:5, 2:5] = 0                                               # here also a point without a slot amid slots: (3, 3, 3)
    opt = _field(sigma, co).optimizer(0.05, 0.01, step=STEP, **{**TV, **tv})
    support = T.support_cells(sigma)
    slots, slot_of, train = G.slot_table(support)
    has = slots.reshape(RES)
    assert np.array_equal(opt.slot_mask.cpu().numpy(), has) and opt.n_slots == int(slots.sum())
    trainable = T.sigma_trainable(support)
    # the slot set has what the test is about: points without a slot next to slots, slots on the lattice faces, sigma that is not trainable
    assert not has[7:].any() and has[6].all() and has[:7, 0].all() and has[:7, :, 0].all() and has[0].all() and has[:7, :, -1].any()
    assert not has[3, 3, 3:].any() and has[2, 3, 3] and has[4, 3, 3] and has[3, 2, 3] and has[3, 4, 3] and has[3, 3, 2]     # slots on 5 sides
    assert (has & ~trainable).any() and trainable.any() and has[0:3, 0:3, 0:3].all()
    rng = np.random.default_rng(11 + degree)
    m = opt._master.cpu().numpy().astype(np.float64)
    assert np.array_equal(m[:, 0] != 0, (m[:, 0] != 0) & train)
    noise = rng.normal(0.0, 0.2, m.shape)
    noise[:, 0] = np.abs(noise[:, 0]) * 3.0 * train
    m = (m + noise).astype(np.float32)
    block = slot_of.reshape(RES)[0:3, 0:3, 0:3].reshape(-1)
    m[block] = m[block[0]]                                                  # 27 equal rows: D = 0 on all axes inside the block
    m[~train, 0] = 0
    m[block, 0] = 0                                                         # (equal in sigma too, whatever is trainable there)
    opt._master.copy_(torch.as_tensor(m))
    return opt, m.astype(np.float64), slot_of, has, trainable


def _dense(rows, has):
    out = np.zeros(has.shape + rows.shape[1:], dtype=rows.dtype)
    out[has] = rows
    return out


def _weights(opt):
    """the per-term weights as the launch receives them: formed in double, passed as float32"""
    ws, wc = opt.tv_weights()
    return float(np.float32(ws)), float(np.float32(wc))


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_tv_gradient_and_value_match_fp64(degree):
    opt, m, slot_of, has, trainable = _tv_setup(degree)
    K = (degree + 1) ** 2
    ws, wc = _weights(opt)
    assert ws == pytest.approx(TV["tv_sigma"] / opt.n_slots, rel=1e-7) and wc == pytest.approx(TV["tv_sh"] / (3 * K * opt.n_slots), rel=1e-7)
    value, grad, sums = G.tv_value_and_grad(m, slot_of, RES, ws, wc, float(np.float32(TV["tv_epsilon"])))
    tv_s, tv_c = opt.regularize()
    assert tv_s.dtype == torch.float64 and tv_s.dim() == 0 and tv_c.dtype == torch.float64 and tv_c.is_cuda
    gs, gc = (g.cpu().numpy() for g in opt.gradients())
    ref_s, ref_c = _dense(grad[:, 0], has), _dense(grad[:, 1:], has).reshape(RES + (K, 3))
    err_s, err_c = float(np.abs(gs - ref_s).max()), float(np.abs(gc - ref_c).max())
    want = (sums[0] / opt.n_slots, sums[1] / (3 * K * opt.n_slots))
    rel = (abs(float(tv_s) - want[0]) / want[0], abs(float(tv_c) - want[1]) / want[1])
    print(f"degree {degree}: max |g - fp64| / w: sigma {err_s / ws / U:.2f} x 2^-24 (max |g| / w {np.abs(ref_s).max() / ws:.2f}), coefficients "
          f"{err_c / wc / U:.2f} x 2^-24 (max |g| / w {np.abs(ref_c).max() / wc:.2f}); bound 64 x 2^-24.  value: relative error "
          f"{rel[0]:.2e} (sigma), {rel[1]:.2e} (coefficients)")
    assert np.abs(ref_s).max() > ws and np.abs(ref_c).max() > wc                     # the gradient is there
    assert np.abs(ref_s[has & ~trainable]).max() > 0                                 # also where sigma is not trainable
    assert (gs[~has] == 0).all() and (gc[~has] == 0).all()
    assert err_s <= 64 * U * ws and err_c <= 64 * U * wc
    assert rel[0] <= 1e-6 and rel[1] <= 1e-6
    # inside the block of equal rows every difference is 0: the terms are sqrt(eps) and the gradient of the centre is exactly 0
    assert gs[1, 1, 1] == 0 and (gc[1, 1, 1] == 0).all() and ref_s[1, 1, 1] == 0 and (ref_c[1, 1, 1] == 0).all()


@pytest.mark.parametrize("degree", [0, 2, 3])
def test_tv_is_one_deterministic_add(degree):
    opt, m, slot_of, has, _ = _tv_setup(degree)
    opt.regularize()
    alone = opt._grad.clone()
    assert float(alone.abs().max()) > 0
    rng = np.random.default_rng(5)
    before = torch.as_tensor(rng.normal(0.0, 1e-4, tuple(alone.shape)).astype(np.float32)).to(alone.device)
    before[::7] = -0.0
    runs = []
    for _ in range(2):
        opt._grad.copy_(before)
        tv = opt.regularize()
        runs.append((opt._grad.clone(), tv))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))                  # two runs: the same bits
    assert torch.equal(runs[0][1][0], runs[1][1][0]) and torch.equal(runs[0][1][1], runs[1][1][1])
    assert torch.equal(runs[0][0], before + alone)                                                  # fp32(before + g), one rounding
    assert torch.equal(runs[0][0].cpu().view(torch.int32), torch.as_tensor((before.cpu().numpy() + alone.cpu().numpy())).view(torch.int32))
    # a weight of exactly 0 leaves the columns of its group untouched, bit for bit (the prefill holds -0.0, which an added +0 would flip)
    for off, cols, rest in (("tv_sigma", slice(0, 1), slice(1, None)), ("tv_sh", slice(1, None), slice(0, 1))):
        saved = getattr(opt, off)
        setattr(opt, off, 0.0)
        opt._grad.copy_(before)
        both = opt.regularize()
        setattr(opt, off, saved)
        after = opt._grad
        assert torch.equal(after[:, cols].view(torch.int32), before[:, cols].view(torch.int32)), off
        assert torch.equal(after[:, rest].view(torch.int32), runs[0][0][:, rest].view(torch.int32)), off
        assert torch.equal(both[0], runs[0][1][0]) and torch.equal(both[1], runs[0][1][1])          # the values are reported all the same


PAIRS = [(RES, FINE), (RES, (12, 9, 8)), (RES, (5, 4, 3)), (RES, (2, 2, 2)), ((2, 2, 2), (4, 3, 5))]


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_resample_is_the_float32_mirror_byte_for_byte(degree):
    rays = _rays(degree)
    for res, res_new in PAIRS:
        sigma, co = _lattice(degree, dense=1.0)
        if res != RES:
            sigma, co = np.ascontiguousarray(sigma[3:5, 3:5, 3:5]), np.ascontiguousarray(co[2:4, 2:4, 2:4])
            sigma[0, 0, 0] = 7.5
        field = _field(sigma, co)
        src = field._records.cpu().numpy()
        assert np.array_equal(src, G.pack(sigma, co, degree))
        for thr in (None, 12.0):
            new = field.resample(res_new, sigma_threshold=thr)
            s, _, want = G.resample(src, res, res_new, degree, 0.0 if thr is None else thr, np.float32)
            got = new._records.cpu().numpy()
            assert got.shape == want.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), (res, res_new, thr, int((got != want).sum()))         # every byte, padding included
            assert new.resolution == tuple(res_new) and new.bounds == field.bounds and new.sh_degree == degree
            assert new.sigma_threshold == (field.sigma_threshold if thr is None else thr)
            if thr is not None:
                assert ((s == 0) | (s > thr)).all()
            from keras_nerf_amd.runtime import occupancy_words_from_grid
            assert torch.equal(new._words, occupancy_words_from_grid(new.sigma, 0.0, 0))
            assert np.array_equal(new.occupied.cpu().numpy(), R.occupied_cells(s))
            a = new.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, skip_empty=True, stats=True)
            b = new.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, skip_empty=False, stats=True)
            for key in ("image", "depth", "opacity"):
                assert torch.equal(a[key], b[key]), (res, res_new, thr, key)
            assert int(a["stats"][0]) <= int(b["stats"][0])
        assert np.array_equal(field._records.cpu().numpy(), src)                                    # the source is left as it is
    # R' = 2 R - 1 through the package: every old point keeps its values
    sigma, co = _lattice(degree, dense=1.0)
    fine = _field(sigma, co).resample(_refined(RES))
    assert np.array_equal(fine.sigma.cpu().numpy()[::2, ::2, ::2], sigma)
    assert np.array_equal(fine.coefficients.cpu().numpy()[::2, ::2, ::2].astype(np.float32), co.astype(np.float32))


def _refined(res):
    from keras_nerf_amd.baked import refined_resolution
    assert refined_resolution(res) == tuple(2 * r - 1 for r in res)
    return refined_resolution(res)


def test_uniform_field():
    from keras_nerf_amd.baked import BakedField
    f = BakedField.uniform((5, 4, 3), (LO, HI), 2, sigma=0.25, colour=0.5)
    assert f.device.type == "cuda" and f.resolution == (5, 4, 3) and f.sh_degree == 2 and f.sigma_threshold == 0.0
    co = np.zeros((5, 4, 3, 9, 3), dtype=np.float16)
    co[..., 0, :] = np.float16(0.5 * 2.0 * np.sqrt(np.pi))
    assert np.array_equal(f._records.cpu().numpy(), G.pack(np.full((5, 4, 3), 0.25, dtype=np.float32), co, 2))
    assert f.occupied.all()
    rays = _rays(2)
    img = f.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, outputs=("image", "opacity"))
    hit = img["opacity"] > 1e-3
    assert hit.sum() > 80                                                                           # grey wherever the box is hit
    assert float((img["image"][hit] / img["opacity"][hit][:, None] - 0.5).abs().max()) < 2e-3       # the DC term alone: colour 0.5
    assert not BakedField.uniform(4, (LO, HI), 0, sigma=0.0).occupied.any()


def test_regularised_step():
    case = _case()
    rays, has = case["rays"], T.slot_points(case["support"])
    make = lambda **kw: _field(case["sigma"], case["co"]).optimizer(0.05, 0.01, step=STEP, **kw)
    # train_step with a weight > 0 is accumulate, regularize, apply: the gradient apply() consumes against fp64
    a = make(**TV)
    calls, seen = [], {}
    acc, reg, app = a.accumulate, a.regularize, a.apply
    a.accumulate = lambda *x, **k: (calls.append("accumulate"), acc(*x, **k))[1]
    a.regularize = lambda *x, **k: (calls.append("regularize"), reg(*x, **k))[1]
    a.apply = lambda *x, **k: (calls.append("apply"), seen.update(g=[t.cpu().numpy() for t in a.gradients()]), app(*x, **k))[-1]
    m0 = a._master.cpu().numpy().astype(np.float64)
    loss = a.train_step(*_batch(rays))
    assert calls == ["accumulate", "regularize", "apply"] and a.iterations == 1 and float(a._grad.abs().max()) == 0.0
    assert abs(float(loss) - case["L"]) <= 1e-5 * case["L"]                                         # the data term alone
    b = make(**TV)
    b.accumulate(*_batch(rays))
    tv_b = b.regularize()
    ws, wc = _weights(b)
    _, slot_of, _ = G.slot_table(case["support"])
    _, tvg, sums = G.tv_value_and_grad(m0, slot_of, RES, ws, wc, float(np.float32(TV["tv_epsilon"])))
    ref_s = case["gs"] + _dense(tvg[:, 0], has)
    ref_c = case["gc"] + _dense(tvg[:, 1:], has).reshape(case["gc"].shape)
    tol_s, tol_c = case["bound"][0] + 64 * U * ws, case["bound"][1] + 64 * U * wc
    for name, (gs, gc) in (("train_step", seen["g"]), ("by hand", [t.cpu().numpy() for t in b.gradients()])):
        err = (float(np.abs(gs - ref_s).max()), float(np.abs(gc - ref_c).max()))
        print(f"{name}: max |g - fp64| sigma {err[0]:.3e} (bound {tol_s:.3e}), coefficients {err[1]:.3e} (bound {tol_c:.3e}); TV share of "
              f"max |g|: {np.abs(tvg[:, 0]).max() / np.abs(ref_s).max():.2f}, {np.abs(tvg[:, 1:]).max() / np.abs(ref_c).max():.2f}")
        assert err[0] <= tol_s and err[1] <= tol_c, name
    assert abs(float(tv_b[0]) - sums[0] / b.n_slots) <= 1e-6 * sums[0] / b.n_slots
    assert abs(float(a.last_regularizer[0]) - float(tv_b[0])) == 0.0 and abs(float(a.last_regularizer[1]) - float(tv_b[1])) == 0.0
    hist = make(**TV).fit([(rays["target"], (rays["o"], rays["d"], None))] * 3, rays["near"], rays["far"])
    assert sorted(hist) == ["loss", "tv_sh", "tv_sigma"] and len(hist["tv_sigma"]) == 3 and len(hist["tv_sh"]) == 3
    assert hist["tv_sigma"][0] == float(tv_b[0]) and hist["tv_sh"][0] == float(tv_b[1])
    # both weights 0: no new launch, and 3 steps give the records of an optimiser built without the keywords, up to the order in which
    # the rays' atomics arrive: 4 x the float32 reference's own deviation between ray orders (plus, for a coefficient, one fp16 step)
    zero, plain = make(tv_sigma=0.0, tv_sh=0.0), make()
    zero.regularize = lambda *x, **k: pytest.fail("regularize() with both weights 0")
    for opt in (zero, plain):
        h = opt.fit([(rays["target"], (rays["o"], rays["d"], None))] * 3, rays["near"], rays["far"])
        assert sorted(h) == ["loss"] and opt.iterations == 3
    ref = lambda order: G.optimise(case["sigma"], case["co"], LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP, rays["target"],
                                   0.05, 0.01, 3, dtype=np.float32, order=order)[3]
    rng = np.random.default_rng(4)
    w_id = ref(None)
    dev = [np.abs(ref(rng.permutation(N_RAYS)) - w_id) for _ in range(3)]
    dev_s, dev_c = max(float(d[:, 0].max()) for d in dev), max(float(d[:, 1:].max()) for d in dev)
    s0, s1 = zero.field.sigma.cpu().numpy(), plain.field.sigma.cpu().numpy()
    c0, c1 = (o.field.coefficients.cpu().numpy().astype(np.float64) for o in (zero, plain))
    half_step = 2.0 ** -10 * np.maximum(np.maximum(np.abs(c0), np.abs(c1)), 2.0 ** -14)
    print(f"weights 0 against no keywords after 3 steps: sigma differs by {np.abs(s0 - s1).max():.3e} (bound {4 * dev_s:.3e}), coefficients "
          f"by {np.abs(c0 - c1).max():.3e} (bound {4 * dev_c:.3e} + one fp16 step)")
    assert np.abs(s0 - s1).max() <= 4 * dev_s and (np.abs(c0 - c1) <= 4 * dev_c + half_step).all()
    assert np.abs(s0 - case["sigma"]).max() > 0.05


@pytest.mark.parametrize("dilation", [0, 1])
def test_nothing_leaves_the_support_with_tv_on(dilation):
    """the assertions of test_gpu_baked_train.py test_nothing_leaves_the_support, 20 steps with the regulariser on and a sigma rate of 2"""
    degree = 2
    case = _case()
    rays = case["rays"]
    support = T.support_cells(case["sigma"], dilation)
    slots, train = T.slot_points(support), T.sigma_trainable(support)
    opt = _field(case["sigma"], case["co"]).optimizer(2.0, 0.05, step=STEP, dilation=dilation, **TV)
    assert np.array_equal(opt.field.occupied.cpu().numpy(), support)
    assert np.array_equal(opt.slot_mask.cpu().numpy(), slots) and np.array_equal(opt.sigma_trainable.cpu().numpy(), train)
    assert opt.n_slots == int(slots.sum()) and not slots.all() and 0 < train.sum() < slots.sum()
    opt.regularize()
    gs, gc = (g.cpu().numpy() for g in opt.gradients())
    assert (gs[~slots] == 0).all() and (gc[~slots] == 0).all() and np.abs(gs[train]).max() > 0 and np.abs(gc[slots]).max() > 0
    # TV reaches the fixed sigma too (with dilation 1 every fixed sigma lies amid zeros: no difference, no gradient)
    assert np.abs(gs[slots & ~train]).max() > 0 or dilation
    opt.accumulate(*_batch(rays))
    opt.apply()
    for k in range(20):
        if k:
            opt.train_step(*_batch(rays))
        a = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, skip_empty=True, stats=True)
        b = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, skip_empty=False, stats=True)
        for key in ("image", "depth", "opacity"):
            assert torch.equal(a[key], b[key]), (k, key)
        assert int(a["stats"][0]) < int(b["stats"][0])
    assert opt.iterations == 20
    sigma = opt.field.sigma.cpu().numpy()
    assert (sigma[~train] == 0).all() and (sigma >= 0).all() and np.isfinite(sigma).all()
    assert np.abs(sigma[train] - case["sigma"][train]).max() > 1.0
    assert (opt._master[:, 0].cpu().numpy()[~train.reshape(-1)[slots.reshape(-1)]] == 0).all()      # the master of a fixed sigma stays 0
    rec = opt.field._records.cpu().numpy()
    used = 4 + 6 * (degree + 1) ** 2
    assert rec.shape[1] > used and (rec[:, used:] == 0).all()
    co = opt.field.coefficients.cpu().numpy()
    assert np.array_equal(co[~slots].view(np.uint16), case["co"][~slots].view(np.uint16))
    assert (co[slots].astype(np.float32) != case["co"][slots].astype(np.float32)).mean() > 0.5


C2F = dict(tv_sigma=1e-3, tv_sh=1e-3, tv_epsilon=1e-6)
C2F_RATES = (0.05, 0.01)
C2F_STAGES = [(None, 20), (FINE, 20)]


def _c2f_setup():
    """(start sigma, start coefficients on RES, rays, targets): field A lives on FINE (the lattice of _lattice refined, so that its
    resample onto RES is that lattice again); the targets are A's fp64 image; the start is A on RES with sigma x 0.7"""
    sigma, co = _lattice(2)
    rays = _rays(2)
    sa, _, ra = G.resample(G.pack(sigma, co, 2), RES, FINE, 2)
    ca = G.unpack(ra, 2)[1].reshape(FINE + (9, 3))
    target = R.march(sa, ca.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP)[0].astype(np.float32)
    return sa.astype(np.float32), ca, rays, target


def _reference_ratio(sa, ca, rays, target):
    """(first loss, last loss, their ratio) of the NumPy loop on the same start and schedule, float64 (about a second on the CPU)"""
    s0, _, r0 = G.resample(G.pack(sa, ca, 2), FINE, RES, 2)
    c0 = G.unpack(r0, 2)[1].reshape(RES + (9, 3))
    losses, final, _, _ = G.fit_coarse_to_fine((s0 * np.float32(0.7)).astype(np.float32), c0, LO, HI, rays["o"], rays["d"], rays["near"],
                                               rays["far"], STEP, target, C2F_STAGES, *C2F_RATES, **C2F)
    return losses[0], final, final / losses[0]


def test_coarse_to_fine(tmp_path):
    from keras_nerf_amd.baked import BakedField
    from keras_nerf_amd.baked_train import fit_coarse_to_fine
    sa, ca, rays, target = _c2f_setup()
    A = _field(sa, ca)
    coarse = A.resample(RES)
    sigma, co = _lattice(2)
    assert np.array_equal(coarse.sigma.cpu().numpy(), sigma) and np.array_equal(coarse.coefficients.cpu().numpy().view(np.uint16), co.view(np.uint16))
    start = _field(sigma * np.float32(0.7), co)
    batches = iter([(target, (rays["o"], rays["d"], None))] * 45)
    done, hist = fit_coarse_to_fine(start, batches, rays["near"], rays["far"], C2F_STAGES, learning_rate_sigma=C2F_RATES[0],
                                    learning_rate_sh=C2F_RATES[1], step=STEP, **C2F)
    assert len(list(batches)) == 5                                                                  # 40 batches were consumed, none dropped
    assert type(done) is BakedField and done.resolution == FINE
    assert len(hist["loss"]) == 40 and len(hist["tv_sigma"]) == 40 and len(hist["tv_sh"]) == 40
    assert [s["resolution"] for s in hist["stages"]] == [RES, FINE] and [s["steps"] for s in hist["stages"]] == [20, 20]
    assert hist["stages"][1]["n_slots"] > hist["stages"][0]["n_slots"]
    img = done.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, outputs="image")["image"]
    final = float(((img - torch.as_tensor(target).to(img.device)).to(torch.float64) ** 2).mean())
    ratio = final / hist["loss"][0]
    ref = _reference_ratio(sa, ca, rays, target)
    print(f"loss {hist['loss'][0]:.4e} -> {final:.4e}: ratio {ratio:.4e} (NumPy loop {ref[0]:.4e} -> {ref[1]:.4e}: ratio {ref[2]:.4e}); loss "
          f"at the resample {hist['loss'][19]:.4e} -> {hist['loss'][20]:.4e}")
    assert abs(hist["loss"][0] - ref[0]) <= 1e-5 * ref[0] and ref[2] < 0.05                         # the same start, and the loop does optimise
    assert ratio <= 2.0 * ref[2]
    assert torch.equal(start.sigma.cpu(), torch.as_tensor(sigma * np.float32(0.7)))                 # the start is untouched
    assert np.array_equal(done.occupied.cpu().numpy(), R.occupied_cells(done.sigma.cpu().numpy()))
    done.save(tmp_path / "grown.npz")
    back = BakedField.load(tmp_path / "grown.npz")
    a = done.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP)
    b = back.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP)
    c = done.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, skip_empty=False)
    for key in ("image", "depth", "opacity"):
        assert torch.equal(a[key], b[key]) and torch.equal(a[key], c[key]), key


def test_arguments_are_refused_before_any_launch():
    from keras_nerf_amd import _lib
    from keras_nerf_amd.baked import _stream
    from keras_nerf_amd.runtime import _ptr
    sigma, co = _lattice(1)
    field = _field(sigma, co)
    for kw in (dict(tv_sigma=-1e-3), dict(tv_sh=float("nan")), dict(tv_epsilon=0.0), dict(tv_epsilon=-1.0), dict(tv_sigma="1")):
        with pytest.raises(ValueError, match="tv_"):
            field.optimizer(0.05, 0.01, **kw)
    for bad in (1, 1026, (9, 7), (9, 7, 0)):
        with pytest.raises(ValueError, match="resolution"):
            field.resample(bad)
    with pytest.raises(ValueError, match="sigma_threshold"):
        field.resample(5, sigma_threshold=-1.0)
    with pytest.raises(ValueError, match="stage"):
        from keras_nerf_amd.baked_train import fit_coarse_to_fine
        fit_coarse_to_fine(field, [], 0.0, 1.0, [], learning_rate_sigma=0.05, learning_rate_sh=0.01)
    # the entry points themselves, on live buffers: refused, and the gradient rows / the destination keep their bytes
    lib, INV = _lib.load(), _lib.KNERF_ERR_INVALID
    opt = field.optimizer(0.05, 0.01, **TV)
    opt._grad.fill_(0.25)
    tv = torch.full((opt.n_slots, 2), -3.0, device=field.device)
    call = lambda c=None, point_of=opt._point_of, master=opt._master, ws=1e-3, wc=1e-3, eps=1e-6: lib.knerf_baked_train_tv(
        _stream(field.device), C.byref(c if c is not None else opt._c), _ptr(point_of), _ptr(master), ws, wc, eps, _ptr(tv))
    broken = _lib.KnerfBakedTrain(opt.field._c, C.c_void_p(opt._slot_of.data_ptr()), C.c_void_p(opt._grad.data_ptr()), 9 * 7 * 6 + 1)
    no_grad = _lib.KnerfBakedTrain(opt.field._c, C.c_void_p(opt._slot_of.data_ptr()), None, opt.n_slots)
    for bad in (dict(point_of=None), dict(master=None), dict(ws=-1e-3), dict(wc=float("nan")), dict(ws=float("inf")), dict(eps=0.0),
                dict(eps=float("nan")), dict(eps=-1e-6), dict(c=broken), dict(c=no_grad)):
        assert call(**bad) == INV, bad
    torch.cuda.synchronize()
    assert bool((opt._grad == 0.25).all()) and bool((tv == -3.0).all())
    dst = torch.full((17 * 13 * 11, 32), 0xAB, device=field.device, dtype=torch.uint8)
    res = lambda f=field._c, new=FINE, thr=0.0, out=dst: lib.knerf_baked_resample(_stream(field.device), C.byref(f), (C.c_int32 * 3)(*new), thr,
                                                                                    _ptr(out))
    wrong = _lib.KnerfBakedField(C.c_void_p(field._records.data_ptr()), None, (C.c_int32 * 3)(9, 7, 6), 5, (C.c_float * 3)(*LO), (C.c_float * 3)(*HI))
    inside = dst[100:]                                                                              # a source inside the destination
    over = _lib.KnerfBakedField(C.c_void_p(inside.data_ptr()), None, (C.c_int32 * 3)(9, 7, 6), 1, (C.c_float * 3)(*LO), (C.c_float * 3)(*HI))
    for bad in (dict(new=(1, 13, 11)), dict(new=(17, 13, 1026)), dict(thr=-1.0), dict(thr=float("nan")), dict(out=None), dict(f=wrong),
                dict(f=over)):
        assert res(**bad) == INV, bad
    assert lib.knerf_baked_resample(_stream(field.device), C.byref(field._c), (C.c_int32 * 3)(9, 7, 6), 0.0, _ptr(field._records)) == INV
    torch.cuda.synchronize()
    assert bool((dst == 0xAB).all())
    assert res() == 0                                                                               # and the good call does write
    assert np.array_equal(dst.cpu().numpy(), G.resample(field._records.cpu().numpy(), RES, FINE, 1)[2])
