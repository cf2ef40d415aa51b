"""Optimising a baked field on the GPU (keras_nerf_amd/baked_train.py, csrc/baked_train.hip) against tests/baked_train_reference.py: the
gradient launch for every SH degree and lane variant on a thin and an opaque lattice, the loss, the support invariant over twenty
steps, one Adam step bit for bit, a short optimisation, and the surface (train_step, accumulate, finish).

Every gradient case first asserts preconditions on the fp64 reference alone (MARGIN = 1e-4): every fetched sample's raw colour channel
and every ray's output before its clamp keep that distance from 0 and 1, at degree >= 1 at least 1 % of the colour channels are
clamped, and with termination no transmittance lies within 0.1 % of the threshold.  The output condition is asserted for the rays with
opacity > 0: a ray that fetches nothing, or only samples of zero density, has the output bg exactly, in the kernel as in the
reference, so its gate cannot differ between them (the ray set has to contain rays that miss).  SEEDS were chosen on the CPU so that
these hold; no element is excluded from a comparison.

Bound per gradient tensor: max(1e-5 x max |g_fp64|, 4 x max over 8 random ray orders of |fp32 reference - fp64 reference|).
Measured on an MI355X, largest over the five cases and every lane variant of a degree, as a share of max |g_fp64| of the tensor
(the bound is 1e-5 of it in every case: 4 x the fp32 reference's own deviation stays below that):
  degree 0: sigma 8.5e-7, coefficients 6.7e-7 (fp32 reference itself 7.5e-7 / 7.6e-7)
  degree 1: sigma 1.5e-6, coefficients 7.9e-7 (1.5e-6 / 8.3e-7)
  degree 2: sigma 1.2e-6, coefficients 9.1e-7 (7.9e-7 / 8.5e-7)
  degree 3: sigma 1.4e-6, coefficients 1.1e-6 (9.3e-7 / 1.0e-6)
i.e. 0.07 ... 0.15 of the bound; the atomics' arrival order costs no more than the reference's own ray order does.
One optimiser step (thin lattice, white background): sigma off the fp64 step by 4.3e-7 (degree 0, 2, 3 at step 1) and 2.1e-7 (degree 2,
step 3), equal to the fp32 mirror's own deviation; coefficients within the mirror's 1.8e-7 of an fp16 rounding boundary: 1 of 882,
62 of 7,938, 141 of 14,112 and 39 of 7,938 (under 1 %), every other half identical.
It optimises: the NumPy reference brings the loss from 8.03e-3 to 2.90e-5 in 40 steps (ratio 3.61e-3); the GPU 8.0318e-3 -> 2.8985e-5.
"""
import numpy as np
import pytest
import torch

from tests import baked_reference as R
from tests import baked_train_reference as T

pytestmark = pytest.mark.gpu

RES = (9, 7, 6)
LO, HI = (-1.0, -0.8, -0.6), (1.0, 0.8, 0.7)
STEP = 0.04
N_RAYS = 150
MARGIN = 1e-4
THIN, OPAQUE = 0.1, 1.0
TERMINATION = 1e-2
VARIANTS = {0: (0, 1), 1: (0, 1, 2), 2: (0, 1, 4), 3: (0, 1, 4)}      # lanes_per_ray values per degree (0: the default)
SEEDS = {0: 1, 1: 1, 2: 1, 3: 2}                                       # per degree: chosen on the CPU until the preconditions hold
COEF_SCALE = {0: 0.6, 1: 0.6, 2: 0.4, 3: 0.3}        # about 1-10 % of the colour channels beyond a clamp edge, few close to one

def _lattice(degree, dense):
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
    aim[:, 0] = rng.uniform(-0.9, 0.2, N_RAYS)                             # at the part of the box that holds density
    d = unit(aim - o)
    near, far = rng.uniform(0.0, 0.5, N_RAYS), rng.uniform(5.0, 6.5, N_RAYS)
    d[90:110] = unit(o[90:110] - mid + 0.3 * rng.standard_normal((20, 3)))
    o[110:130] = rng.uniform(lo + 0.05, hi - 0.05, (20, 3)); d[110:130] = unit(rng.standard_normal((20, 3))); near[110:130] = 0.0
    for i in range(130, 138):                                              # one component exactly 0
        a = i % 3
        t = rng.uniform(lo + 0.2, hi - 0.2)
        o[i][a] = t[a]
        d[i] = t - o[i]; d[i][a] = 0.0; d[i] = unit(d[i])
    for i in range(138, 142):                                              # parallel to an axis
        a = i % 3
        o[i] = rng.uniform(lo + 0.2, hi - 0.2); d[i] = 0.0; d[i][a] = 1.0 if i % 2 else -1.0
        o[i][a] = mid[a] - 3.0 * d[i][a]
    for i, s in zip(range(142, 150), (2.5, 0.3, 7.0, 1.0 / 3.0, 1.7, 0.6, 4.0, 0.45)):
        d[i] *= s; near[i] /= s; far[i] /= s
    target = rng.uniform(0.0, 1.0, (N_RAYS, 3))
    return {"o": o.astype(np.float32), "d": d.astype(np.float32), "near": near.astype(np.float32), "far": far.astype(np.float32),
            "target": target.astype(np.float32)}


_cases = {}


def _case(degree, dense, white, termination=0.0):
    """lattice, rays, the fp64 reference with its preconditions checked, and the bounds: computed once per case and shared"""
    key = (degree, dense, white, termination)
    if key in _cases:
        return _cases[key]
    sigma, co = _lattice(degree, dense)
    rays = _rays(degree)
    support = T.support_cells(sigma)
    args = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP, rays["target"], support, white,
            termination)
    info = {}
    L, gs, gc, out = T.loss_and_grad(*args, info=info)
    raw, pre, opa, Tn = info["raw"], info["pre"], info["opacity"], info["T"]
    assert raw.shape[0] > 1500 and (opa[:90] > 0.05).all() and (opa[90:110] == 0).all()             # the set does what it says
    assert min(np.abs(raw).min(), np.abs(raw - 1).min()) >= MARGIN, (degree, "a raw colour on a clamp edge")
    clamped = float(((raw < 0) | (raw > 1)).mean())
    assert degree == 0 or clamped >= 0.01, (degree, clamped)
    hit = opa > 0
    assert min(np.abs(pre[hit]).min(), np.abs(pre[hit] - 1).min()) >= MARGIN, (key, "an output on a clamp edge")
    assert (pre[~hit] == (1.0 if white else 0.0)).all()
    if termination:
        assert (Tn < termination).sum() >= 20 and np.abs(Tn / termination - 1).min() >= 1e-3, (key, "a transmittance on the threshold")
    if dense == THIN and not termination:
        assert np.median(1 - opa[:90]) > 1e-3                              # light reaches the far side: the gradient behind is visible
    dev_s = dev_c = 0.0
    rng = np.random.default_rng(99)
    for _ in range(8):                                                     # the fp32 reference's own error over 8 accumulation orders
        _, s32, c32, _ = T.loss_and_grad(*args, dtype=np.float32, order=rng.permutation(N_RAYS))
        dev_s, dev_c = max(dev_s, float(np.abs(s32 - gs).max())), max(dev_c, float(np.abs(c32 - gc).max()))
    bound = (max(1e-5 * float(np.abs(gs).max()), 4.0 * dev_s), max(1e-5 * float(np.abs(gc).max()), 4.0 * dev_c))
    _cases[key] = {"sigma": sigma, "co": co, "rays": rays, "support": support, "L": L, "gs": gs, "gc": gc, "out": out, "bound": bound,
                   "clamped": clamped, "dev": (dev_s, dev_c)}
    return _cases[key]


def _field(case):
    from keras_nerf_amd.baked import BakedField
    return BakedField.from_arrays(case["sigma"], case["co"], (LO, HI))


def _optimizer(case, white=False, termination=0.0, lanes=0, lr_sigma=0.05, lr_sh=0.01, **kw):
    return _field(case).optimizer(lr_sigma, lr_sh, step=STEP, white_background=white, termination=termination, lanes_per_ray=lanes, **kw)


def _batch(rays, sl=slice(None)):
    return rays["o"][sl], rays["d"][sl], rays["near"][sl], rays["far"][sl], rays["target"][sl]


CASES = [(deg, dense, white, 0.0) for deg in (0, 1, 2, 3) for dense in (THIN, OPAQUE) for white in (False, True)] + \
    [(deg, OPAQUE, deg % 2 == 1, TERMINATION) for deg in (0, 1, 2, 3)]


@pytest.mark.parametrize("degree,dense,white,termination", CASES)
def test_gradient_matches_fp64(degree, dense, white, termination):
    case = _case(degree, dense, white, termination)
    slots = T.slot_points(case["support"])
    for lanes in VARIANTS[degree]:
        opt = _optimizer(case, white, termination, lanes)
        assert np.array_equal(opt.slot_mask.cpu().numpy(), slots)
        loss = opt.accumulate(*_batch(case["rays"]))
        gs, gc = (g.cpu().numpy() for g in opt.gradients())
        assert loss.dtype == torch.float64 and loss.dim() == 0
        assert abs(float(loss) - case["L"]) <= 1e-5 * case["L"]
        err = (float(np.abs(gs - case["gs"]).max()), float(np.abs(gc - case["gc"]).max()))
        print(f"degree {degree} dense {dense} white {white} termination {termination} lanes {lanes}: max |g - fp64| sigma {err[0]:.3e} "
              f"(bound {case['bound'][0]:.3e}, fp32 reference {case['dev'][0]:.3e}, max |g| {np.abs(case['gs']).max():.3e}), coefficients "
              f"{err[1]:.3e} (bound {case['bound'][1]:.3e}, fp32 reference {case['dev'][1]:.3e}, max |g| {np.abs(case['gc']).max():.3e}); "
              f"clamped {case['clamped']:.3%}")
        assert gs.dtype == np.float32 and gs.shape == RES and gc.shape == RES + ((degree + 1) ** 2, 3)
        assert (gs[~slots] == 0).all() and (gc[~slots] == 0).all()
        assert err[0] <= case["bound"][0], (lanes, "sigma", err[0], case["bound"][0])
        assert err[1] <= case["bound"][1], (lanes, "coefficients", err[1], case["bound"][1])


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_loss_is_the_mse_of_the_rendered_image(degree):
    for dense, white, termination in ((THIN, True, 0.0), (OPAQUE, False, TERMINATION)):
        case = _case(degree, dense, white, termination)
        rays = case["rays"]
        for lanes in VARIANTS[degree]:
            opt = _optimizer(case, white, termination, lanes)
            loss = float(opt.accumulate(*_batch(rays)))
            img = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, white_background=white,
                                   termination=termination, lanes_per_ray=lanes, outputs="image")["image"]
            tg = torch.as_tensor(rays["target"]).to(img.device)
            mse = float(((img - tg).to(torch.float64) ** 2).mean())
            assert abs(loss - mse) <= 1e-6 * mse, (degree, lanes, loss, mse)


@pytest.mark.parametrize("dilation", [0, 1])
def test_nothing_leaves_the_support(dilation):
    """after 20 steps with a large sigma rate: sigma is exactly 0 wherever it is not trainable and >= 0 everywhere, the records'
    padding is zero, and rendering with and without skipping stays bit-identical at every step"""
    degree = 2
    case = _case(degree, THIN, False)
    rays = case["rays"]
    support = T.support_cells(case["sigma"], dilation)
    slots, train = T.slot_points(support), T.sigma_trainable(support)
    opt = _optimizer(case, lr_sigma=2.0, lr_sh=0.05, dilation=dilation)
    assert np.array_equal(opt.field.occupied.cpu().numpy(), support)
    assert np.array_equal(opt.slot_mask.cpu().numpy(), slots) and np.array_equal(opt.sigma_trainable.cpu().numpy(), train)
    assert opt.n_slots == int(slots.sum()) and not slots.all() and 0 < train.sum() < slots.sum()
    opt.accumulate(*_batch(rays))
    gs, gc = (g.cpu().numpy() for g in opt.gradients())
    assert (gs[~slots] == 0).all() and (gc[~slots] == 0).all() and np.abs(gs[slots & ~train]).max() > 0
    opt.apply()
    start = case["sigma"]
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
    assert np.abs(sigma[train] - start[train]).max() > 1.0                  # and the rate did move it
    rec = opt.field._records.cpu().numpy()
    used = 4 + 6 * (degree + 1) ** 2
    assert rec.shape[1] > used and (rec[:, used:] == 0).all()
    co = opt.field.coefficients.cpu().numpy()
    assert np.array_equal(co[~slots].view(np.uint16), case["co"][~slots].view(np.uint16))        # records without a slot keep their bytes
    assert (co[slots].astype(np.float32) != case["co"][slots].astype(np.float32)).mean() > 0.5


def _rows(opt):
    return tuple(x.cpu().numpy().astype(np.float64) for x in (opt._master, opt._m, opt._v, opt._grad))


@pytest.mark.parametrize("degree,before", [(0, 0), (2, 0), (3, 0), (2, 2)])
def test_one_optimiser_step(degree, before):
    """the records after apply() against the fp64 Adam + projection + repack fed the GPU's own gradient; before = 2: step 3 of a run"""
    case = _case(degree, THIN, True)
    rays = case["rays"]
    lr_s, lr_c = 0.05, 0.01
    opt = _optimizer(case, white=True, lr_sigma=lr_s, lr_sh=lr_c)
    for _ in range(before):
        opt.train_step(*_batch(rays))
    opt.accumulate(*_batch(rays))
    w, m, v, g = _rows(opt)
    slots = opt.slot_mask.cpu().numpy().reshape(-1)
    gs, gc = (x.cpu().numpy() for x in opt.gradients())
    K = (degree + 1) ** 2
    assert np.array_equal(g, np.concatenate([gs.reshape(-1, 1)[slots], gc.reshape(-1, 3 * K)[slots]], axis=1).astype(np.float64))
    train = opt.sigma_trainable.cpu().numpy().reshape(-1)[slots]
    t = before + 1
    hyper = (train, lr_s, lr_c, 0.9, 0.999, 1e-7, t)
    w64, m64, v64, s64, c16 = T.adam_step(w, m, v, g, *hyper)
    w32 = T.adam_step(w, m, v, g, *hyper, dtype=np.float32)[0].astype(np.float64)
    dev_s = float(np.abs(w32[:, 0] - w64[:, 0]).max())
    dev_c = float(np.abs(w32[:, 1:] - w64[:, 1:]).max())
    opt.apply()
    assert opt.iterations == t
    sigma = opt.field.sigma.cpu().numpy().reshape(-1)[slots].astype(np.float64)
    co = opt.field.coefficients.cpu().numpy().reshape(-1, 3 * K)[slots]
    err_s = float(np.abs(sigma - w64[:, 0]).max())
    lo16, hi16 = (w64[:, 1:] - dev_c).astype(np.float16), (w64[:, 1:] + dev_c).astype(np.float16)
    near_boundary = lo16.view(np.uint16) != hi16.view(np.uint16)
    share = float(near_boundary.mean())
    print(f"degree {degree} step {t}: max |sigma - fp64| {err_s:.3e} (fp32 mirror {dev_s:.3e}); coefficients: fp32 mirror {dev_c:.3e}, "
          f"{int(near_boundary.sum())} of {near_boundary.size} within that of an fp16 rounding boundary")
    assert share < 0.01                                                    # the precondition on the reference
    assert err_s <= max(4.0 * dev_s, 2.0 ** -24 * float(np.abs(w64[:, 0]).max())), (err_s, dev_s)
    bits = co.view(np.uint16)
    assert np.array_equal(bits[~near_boundary], c16.view(np.uint16)[~near_boundary])
    # there the kernel's half lies between the two (below 2^-14 the halfs are closer together than the deviation: several fit in between)
    assert ((co >= lo16) & (co <= hi16))[near_boundary].all()
    assert (sigma[~train] == 0).all() and (sigma >= 0).all()
    assert float(opt._grad.abs().max()) == 0.0                             # the gradient rows are zero afterwards
    w1, m1, v1, _ = _rows(opt)
    # the moments: fp32(1 - fp32(beta)) is off by up to 2^-24 beta / (1 - beta) of itself, 5.4e-7 for beta_1 and 6.0e-5 for beta_2; twice that
    assert np.abs(m1 - m64).max() <= 1.1e-6 * np.abs(m64).max() and np.abs(v1 - v64).max() <= 1.2e-4 * np.abs(v64).max()
    assert np.array_equal(w1[:, 0], sigma)


REFERENCE_RATIO = 3.61e-3      # final / initial loss (8.03e-3 -> 2.90e-5) of tests/baked_train_reference.py optimise() on the same 40 steps, float64 on the CPU


def test_it_optimises(tmp_path):
    """targets rendered from field A; the start is A with sigma x 0.7 and coefficients x 0.8 plus noise; 40 full-batch steps on the
    thin lattice at degree 2.  The NumPy reference optimiser (float64, run once on the CPU) brings the loss to REFERENCE_RATIO of its
    start; the GPU must reach at most twice that: Adam divides by sqrt(v), which amplifies rounding noise where gradients are tiny."""
    from keras_nerf_amd.baked import BakedField
    sigma, co, rays, target = _optimise_setup()
    start = BakedField.from_arrays(sigma, co, (LO, HI))
    opt = start.optimizer(OPT_RATES[0], OPT_RATES[1], step=STEP)
    batch = (rays["o"], rays["d"], rays["near"], rays["far"], target)
    hist = opt.fit([(torch.as_tensor(target), (rays["o"], rays["d"], None))] * 40, rays["near"], rays["far"])["loss"]
    final = float(opt.accumulate(*batch))
    assert len(hist) == 40 and opt.iterations == 40
    ratio = final / hist[0]
    print(f"loss {hist[0]:.4e} -> {final:.4e}: ratio {ratio:.4f} (reference {REFERENCE_RATIO})")
    assert ratio <= 2.0 * REFERENCE_RATIO
    assert torch.equal(start.sigma.cpu(), torch.as_tensor(sigma))          # the field the optimiser was made from is untouched
    done = opt.finish()
    assert type(done) is BakedField and done.sigma_threshold == start.sigma_threshold
    occ, sup = done.occupied.cpu().numpy(), opt.field.occupied.cpu().numpy()
    assert (occ <= sup).all() and np.array_equal(occ, R.occupied_cells(done.sigma.cpu().numpy()))
    done.save(tmp_path / "tuned.npz")
    back = BakedField.load(tmp_path / "tuned.npz")
    kw = dict(step=STEP, white_background=False)
    a = done.render(rays["o"], rays["d"], rays["near"], rays["far"], **kw)
    b = back.render(rays["o"], rays["d"], rays["near"], rays["far"], **kw)
    c = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], **kw)
    for key in ("image", "depth", "opacity"):
        assert torch.equal(a[key], b[key]) and torch.equal(a[key], c[key]), key
    cut = opt.finish(sigma_threshold=0.5)
    s = cut.sigma.cpu().numpy()
    assert ((s == 0) | (s > 0.5)).all() and (s == 0).sum() > (done.sigma.cpu().numpy() == 0).sum()
    assert np.array_equal(cut.occupied.cpu().numpy(), R.occupied_cells(s))


OPT_RATES = (0.05, 0.01)


def _optimise_setup():
    """(start sigma, start coefficients, rays, targets): the targets are field A's fp64 image"""
    sigma, co = _lattice(2, THIN)
    rays = _rays(2)
    target = R.march(sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP)[0].astype(np.float32)
    rng = np.random.default_rng(5)
    co0 = (co.astype(np.float32) * 0.8 + 0.05 * rng.standard_normal(co.shape)).astype(np.float16)
    return (sigma * np.float32(0.7)).astype(np.float32), co0, rays, target


def test_train_step_is_accumulate_then_apply():
    case = _case(2, THIN, False)
    rays = case["rays"]
    opt = _optimizer(case)
    calls = []
    acc, app = opt.accumulate, opt.apply
    opt.accumulate = lambda *a, **k: (calls.append("accumulate"), acc(*a, **k))[1]
    opt.apply = lambda *a, **k: (calls.append("apply"), app(*a, **k))[1]
    loss = opt.train_step(*_batch(rays))
    assert calls == ["accumulate", "apply"] and opt.iterations == 1
    assert abs(float(loss) - case["L"]) <= 1e-5 * case["L"] and float(opt._grad.abs().max()) == 0.0
    # two half batches normalised by the whole count are the whole batch, within the bound of the gradient test
    other = _optimizer(case)
    l1 = other.accumulate(*_batch(rays, slice(0, 75)), n_total=N_RAYS)
    l2 = other.accumulate(*_batch(rays, slice(75, None)), n_total=N_RAYS)
    gs, gc = (g.cpu().numpy() for g in other.gradients())
    assert abs(float(l1 + l2) - case["L"]) <= 1e-5 * case["L"]
    assert np.abs(gs - case["gs"]).max() <= case["bound"][0] and np.abs(gc - case["gc"]).max() <= case["bound"][1]
    whole = _optimizer(case)
    whole.accumulate(*_batch(rays))
    ws, wc = (g.cpu().numpy() for g in whole.gradients())
    assert np.abs(gs - ws).max() <= 2 * case["bound"][0] and np.abs(gc - wc).max() <= 2 * case["bound"][1]


def test_arguments_are_refused_before_any_launch():
    case = _case(0, THIN, False)
    rays = case["rays"]
    field = _field(case)
    for kw in (dict(learning_rate_sigma=0.0), dict(learning_rate_sh=-1.0), dict(beta_1=1.0), dict(beta_2=-0.5), dict(epsilon=0.0),
               dict(dilation=-1), dict(termination=1.0), dict(step=0.0), dict(lanes_per_ray=4)):
        with pytest.raises(ValueError):
            field.optimizer(**{**dict(learning_rate_sigma=0.05, learning_rate_sh=0.01), **kw})
    opt = _optimizer(case)
    o, d, near, far, tg = _batch(rays)
    for bad in (tg[:100], tg[:, :2], tg.reshape(-1)):
        with pytest.raises(ValueError, match="target"):
            opt.accumulate(o, d, near, far, bad)
    with pytest.raises(ValueError):
        opt.accumulate(o, d[:10], near, far, tg)
    assert float(opt._grad.abs().max()) == 0.0 and opt.iterations == 0
    from keras_nerf_amd.baked import BakedField
    with pytest.raises(ValueError, match="nothing to optimise"):
        BakedField.from_arrays(np.zeros(RES, dtype=np.float32), case["co"], (LO, HI)).optimizer(0.05, 0.01)
