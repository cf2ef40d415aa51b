"""Optimising a brick baked field on the GPU (keras_nerf_amd/baked_bricks_train.py, csrc/baked_train.hip): bit identity with the
dense optimiser of the same field, whole batches against the fp64 reference, the support invariant over twenty steps, a short
optimisation with save / load, the memory condition (no tensor of the dense table's size) and the lane variants.  The conditions are
stated in tests/README_baked_bricks_train.md.  No test feeds the kernel a damaged table: its range guard is checked by reading.

The reference of a brick optimiser over a brick field F is tests/baked_train_reference.py on the dense arrays of F.

Measured on an MI355X:
  bit identity: the precondition (two dense optimisers fed the rays one per launch give equal gradient bits) holds in all 89 cases,
  and so does every equality behind it;
  whole batches, largest over both brick sizes and every lane variant of a degree, as a share of max |g_fp64| of the tensor (the bound
  is 1e-5 of it in every case): degree 0 sigma 1.5e-6, coefficients 1.1e-6; degree 1 1.4e-6 / 1.8e-6; degree 2 1.1e-6 / 1.8e-6;
  degree 3 1.2e-6 / 1.4e-6, i.e. 0.11 ... 0.18 of the bound;
  it optimises: the NumPy reference 2.7738e-3 -> 1.3117e-5 in 40 steps (ratio 4.73e-3), the GPU 2.7738e-3 -> 1.3120e-5;
  no dense table: peak 18.5 MiB above the start at 129^3, where the dense table is 131 MiB;
  all 108 tests together take 17 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from keras_nerf_amd.baked_bricks_train import BRICK_TRAIN_VARIANTS
from tests import baked_bricks_reference as B
from tests import baked_bricks_train_reference as S
from tests import baked_reference as R
from tests import baked_train_reference as T
from tests.test_baked_bricks_host import BRICKS, HI, LO, RES
from tests.test_baked_bricks_train_host import lattice
from tests.test_gpu_baked import N_RAYS, STEP, rays  # noqa: F401 -- the ray set of the dense render tests (a fixture), over the same box

pytestmark = pytest.mark.gpu

TERMINATION = 1e-2
MARGIN = 1e-4
RATES = (0.05, 0.01)
OUT = ("image", "depth", "opacity")
# the lattice of the fp64 comparison, per degree (seed, shrink of tests/test_baked_bricks_train_host.py lattice): chosen on the CPU so
# that the preconditions of _case hold; at degree 3 the coefficients above order 0 are halved (18 % of the colour channels are clamped
# otherwise and no seed of 30 keeps all of them 1e-4 off an edge)
FP64_LATTICE = {0: (0, 1.0), 1: (2, 1.0), 2: (0, 1.0), 3: (0, 0.5)}

_sources, _device_rays = {}, {}


def _source(degree, b, seed=0, shrink=1.0):
    """the brick field of the test lattice, built once and never changed (an optimiser works on a copy)"""
    from keras_nerf_amd.baked import BakedField
    key = (degree, b, seed, shrink)
    if key not in _sources:
        sigma, co = lattice(degree, seed, shrink)
        _sources[key] = BakedField.from_arrays(sigma, co, (LO, HI)).compact(b)
    return _sources[key]


def _targets(degree):
    return np.random.default_rng(40 + degree).uniform(0.0, 1.0, (N_RAYS, 3)).astype(np.float32)


def _on_device(rays, degree):
    if degree not in _device_rays:
        _device_rays[degree] = {k: torch.as_tensor(v).cuda() for k, v in {**rays, "target": _targets(degree)}.items()}
    return _device_rays[degree]


def _batch(r, sl=slice(None)):
    return r["o"][sl], r["d"][sl], r["near"][sl], r["far"][sl], r["target"][sl]


def _feed(opt, r):
    """the rays one per launch: within a launch of one ray every gradient address is added to by one lane in program order, so the
    sums do not depend on arrival order"""
    for i in range(N_RAYS):
        opt.accumulate(*_batch(r, slice(i, i + 1)), n_total=N_RAYS)


def _rows_at(opt, rows, index):
    """rows of a brick optimiser's per-record state at the lattice points `index`"""
    return opt._dense(rows, torch.float32)[index]


IDENTITY_CASES = [(degree, lanes, b, dilation, white, 0.0) for degree in (0, 1, 2, 3) for lanes in (0,) + BRICK_TRAIN_VARIANTS[degree]
                  for b in BRICKS for dilation in (0, 1) for white in (False, True)] + [(2, 0, 8, 1, True, TERMINATION)]


@pytest.mark.parametrize("degree,lanes,b,dilation,white,termination", IDENTITY_CASES)
def test_bit_identity_with_the_dense_optimiser(degree, lanes, b, dilation, white, termination, rays):
    """D = the dense optimiser of bricks.to_dense() (absent bricks hold zero coefficients there), S = the brick optimiser, fed the same
    one-ray accumulations: equal gradients, and after every one of four steps equal records, master values and moments; equal finish()."""
    from keras_nerf_amd.baked_train import brick_optimizer
    src = _source(degree, b)
    r = _on_device(rays, degree)
    kw = dict(step=STEP, white_background=white, termination=termination, lanes_per_ray=lanes, dilation=dilation)
    dense = src.to_dense()
    D, again = dense.optimizer(*RATES, **kw), dense.optimizer(*RATES, **kw)
    _feed(D, r)
    _feed(again, r)
    gD, gA = D.gradients(), again.gradients()
    assert float(gD[0].abs().max()) > 0 and float(gD[1].abs().max()) > 0
    # the precondition: the dense optimiser itself repeats its bits when a launch holds one ray
    assert torch.equal(gD[0], gA[0]) and torch.equal(gD[1], gA[1])
    Sx = brick_optimizer(src, *RATES, **kw)
    assert Sx.n_slots == D.n_slots and torch.equal(Sx.slot_mask, D.slot_mask) and torch.equal(Sx.sigma_trainable, D.sigma_trainable)
    assert (Sx.field.n_bricks > src.n_bricks) == (dilation == 1) and torch.equal(Sx.field._words, D.field._words)
    _feed(Sx, r)
    gS = Sx.gradients()
    assert gS[0].dtype == torch.float32 and gS[0].shape == RES and gS[1].shape == RES + ((degree + 1) ** 2, 3)
    assert torch.equal(gS[0], gD[0]) and torch.equal(gS[1], gD[1])
    for k in range(4):
        if k:
            _feed(D, r)
            _feed(Sx, r)
            (s0, s1), (d0, d1) = Sx.gradients(), D.gradients()
            assert torch.equal(s0, d0) and torch.equal(s1, d1), k
        D.apply()
        Sx.apply()
        assert torch.equal(Sx.field.to_dense()._records, D.field._records), k
        for name in ("_master", "_m", "_v", "_grad"):
            assert torch.equal(_rows_at(Sx, getattr(Sx, name), D._index), getattr(D, name)), (k, name)
    assert Sx.iterations == D.iterations == 4 and float(Sx._grad.abs().max()) == 0.0
    assert not torch.equal(D.field._records, dense._records)              # and the four steps did move the records
    got, want = Sx.finish(), D.finish().compact(b)
    assert torch.equal(got._records, want._records) and torch.equal(got.brick_of, want.brick_of) and torch.equal(got._words, want._words)
    assert got.n_bricks == want.n_bricks and got.sigma_threshold == want.sigma_threshold
    assert torch.equal(src._records, _source(degree, b)._records) and torch.equal(src.to_dense()._records, dense._records)   # the source is untouched


_cases = {}


def _case(degree, white, termination, rays):
    """the fp64 reference on the dense arrays, its preconditions and the bound of tests/test_gpu_baked_train.py
    test_gradient_matches_fp64 -- max(1e-5 max |g|, 4 x the fp32 reference's deviation over 8 ray orders) -- computed once per case.
    Preconditions, asserted on the reference alone: every fetched sample's raw colour channel keeps MARGIN from 0 and 1; so does every
    output before its clamp of a ray with opacity > 0, except an output that is exactly 0 under the black background (every colour of
    that channel is clamped to 0: the sum is exactly 0 in the kernel as well); a ray with opacity 0 has the background exactly; with
    termination no transmittance lies within 0.1 % of the threshold."""
    key = (degree, white, termination)
    if key in _cases:
        return _cases[key]
    sigma, co = lattice(degree, *FP64_LATTICE[degree])
    target = _targets(degree)
    support = T.support_cells(sigma)
    args = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP, target, support, white, termination)
    info = {}
    L, gs, gc, out = T.loss_and_grad(*args, info=info)
    raw, pre, opa, Tn = info["raw"], info["pre"], info["opacity"], info["T"]
    hit = opa > 0
    assert raw.shape[0] > 500 and hit.sum() >= 30 and (~hit).sum() >= 20
    assert min(np.abs(raw).min(), np.abs(raw - 1).min()) >= MARGIN, (key, "a raw colour on a clamp edge")
    edge = np.minimum(np.abs(pre), np.abs(pre - 1))
    assert ((edge >= MARGIN) | ((pre == 0) & (not white)))[hit].all(), (key, "an output on a clamp edge")
    assert (pre[~hit] == (1.0 if white else 0.0)).all()
    if termination:
        assert (Tn < termination).sum() >= 10 and np.abs(Tn / termination - 1).min() >= 1e-3, (key, "a transmittance on the threshold")
    # the brick fields' dense arrays are the lattice at every slot, for both brick sizes: an absent brick holds no corner of the support
    slots = T.slot_points(support)
    for b in BRICKS:
        src = _source(degree, b, *FP64_LATTICE[degree])
        sg, cf = S.dense_arrays(src._records.cpu().numpy(), src.brick_of.cpu().numpy(), RES, b, degree)
        assert np.array_equal(sg, sigma) and np.array_equal(cf[slots].view(np.uint16), co[slots].view(np.uint16))
    dev_s = dev_c = 0.0
    rng = np.random.default_rng(99)
    for _ in range(8):                                                     # the fp32 reference's own error over 8 accumulation orders
        _, s32, c32, _ = T.loss_and_grad(*args, dtype=np.float32, order=rng.permutation(N_RAYS))
        dev_s, dev_c = max(dev_s, float(np.abs(s32 - gs).max())), max(dev_c, float(np.abs(c32 - gc).max()))
    bound = (max(1e-5 * float(np.abs(gs).max()), 4.0 * dev_s), max(1e-5 * float(np.abs(gc).max()), 4.0 * dev_c))
    _cases[key] = {"L": L, "gs": gs, "gc": gc, "bound": bound, "dev": (dev_s, dev_c), "slots": slots, "target": target}
    return _cases[key]


BATCH_CASES = [(degree, white, 0.0) for degree in (0, 1, 2, 3) for white in (False, True)] + \
    [(degree, degree % 2 == 1, TERMINATION) for degree in (0, 1, 2, 3)]


@pytest.mark.parametrize("degree,white,termination", BATCH_CASES)
def test_whole_batches_match_fp64(degree, white, termination, rays):
    from keras_nerf_amd.baked_train import brick_optimizer
    case = _case(degree, white, termination, rays)
    slots = case["slots"]
    batch = (rays["o"], rays["d"], rays["near"], rays["far"], case["target"])
    for b in BRICKS:
        for lanes in (0,) + BRICK_TRAIN_VARIANTS[degree]:
            opt = brick_optimizer(_source(degree, b, *FP64_LATTICE[degree]), *RATES, step=STEP, white_background=white,
                                  termination=termination, lanes_per_ray=lanes)
            assert np.array_equal(opt.slot_mask.cpu().numpy(), slots)
            loss = opt.accumulate(*batch)
            gs, gc = (g.cpu().numpy() for g in opt.gradients())
            assert loss.dtype == torch.float64 and loss.dim() == 0
            err = (float(np.abs(gs - case["gs"]).max()), float(np.abs(gc - case["gc"]).max()))
            print(f"degree {degree} white {white} termination {termination} b {b} lanes {lanes}: max |g - fp64| sigma {err[0]:.3e} (bound "
                  f"{case['bound'][0]:.3e}, fp32 reference {case['dev'][0]:.3e}, max |g| {np.abs(case['gs']).max():.3e}), coefficients "
                  f"{err[1]:.3e} (bound {case['bound'][1]:.3e}, fp32 reference {case['dev'][1]:.3e}, max |g| {np.abs(case['gc']).max():.3e})")
            assert abs(float(loss) - case["L"]) <= 1e-5 * case["L"]
            assert (gs[~slots] == 0).all() and (gc[~slots] == 0).all()
            assert err[0] <= case["bound"][0], (b, lanes, "sigma", err[0], case["bound"][0])
            assert err[1] <= case["bound"][1], (b, lanes, "coefficients", err[1], case["bound"][1])
            # the loss is the mean squared error of the live field's own render
            img = opt.field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, white_background=white,
                                   termination=termination, lanes_per_ray=lanes, outputs="image")["image"]
            mse = float(((img - torch.as_tensor(case["target"]).to(img.device)).to(torch.float64) ** 2).mean())
            assert abs(float(loss) - mse) <= 1e-6 * mse, (degree, b, lanes, float(loss), mse)


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("dilation", [0, 1])
def test_nothing_leaves_the_support(dilation, b, rays):
    """20 steps with a sigma rate of 2.0: rendering the live field with and without skipping stays bit-identical at every step, no
    record of a point without a slot changes, sigma stays 0 wherever it is not trainable, and the brick set stays the train set"""
    from keras_nerf_amd.baked_bricks_train import brick_sigma
    from keras_nerf_amd.baked_train import brick_optimizer
    degree = 2
    sigma0, _ = lattice(degree)
    r = _on_device(rays, degree)
    src = _source(degree, b)
    support, train_of, n = S.train_bricks(sigma0, b, dilation)
    flags = S.flags(support, train_of, b)
    opt = brick_optimizer(src, 2.0, 0.05, step=STEP, dilation=dilation)
    assert np.array_equal(opt.field.occupied.cpu().numpy(), support) and np.array_equal(opt.field.brick_of.cpu().numpy(), train_of)
    assert opt.field.n_bricks == n and np.array_equal(opt._flags.cpu().numpy(), flags) and opt.n_slots == int((flags & 1).sum())
    slots, train = T.slot_points(support), T.sigma_trainable(support)
    assert np.array_equal(opt.slot_mask.cpu().numpy(), slots) and np.array_equal(opt.sigma_trainable.cpu().numpy(), train)
    assert opt.nbytes == opt.field.nbytes + flags.size * (1 + 4 * 4 * 28)
    before, master = opt.field._records.clone(), opt._master.cpu().numpy()
    for k in range(20):
        opt.train_step(*_batch(r))
        a = opt.field.render(*_batch(r)[:4], step=STEP, skip_empty=True, stats=True)
        c = opt.field.render(*_batch(r)[:4], step=STEP, skip_empty=False, stats=True)
        for key in OUT:
            assert torch.equal(a[key], c[key]), (k, key)
        assert int(a["stats"][0]) < int(c["stats"][0])
    assert opt.iterations == 20
    rec, was = opt.field._records.cpu().numpy().reshape(flags.size, -1), before.cpu().numpy().reshape(flags.size, -1)
    slot_row = (flags & 1) != 0
    assert np.array_equal(rec[~slot_row], was[~slot_row]) and (rec[slot_row] != was[slot_row]).any(axis=1).mean() > 0.5
    for rows in (opt._m, opt._v, opt._grad):                               # a row without a slot is never touched
        assert not rows.cpu().numpy()[~slot_row].any()
    assert np.array_equal(opt._master.cpu().numpy()[~slot_row], master[~slot_row]) and opt._m.cpu().numpy()[slot_row].any()
    assert np.array_equal(opt.field.brick_of.cpu().numpy(), train_of)      # bricks outside the train set stay absent
    used = 4 + 6 * (degree + 1) ** 2
    assert rec.shape[1] > used and (rec[:, used:] == 0).all()
    sigma = brick_sigma(opt.field)[1].cpu().numpy()
    assert (sigma[~train] == 0).all() and (sigma >= 0).all() and np.isfinite(sigma).all()
    assert np.abs(sigma[train] - sigma0[train]).max() > 1.0                # and the rate did move it


OPT_RATES = (0.5, 0.01)
REFERENCE_RATIO = 4.73e-3   # final / initial loss (2.7738e-3 -> 1.3117e-5) of tests/baked_train_reference.py optimise() on the dense arrays of
# the start field's bricks, the same 40 steps and rates, float64 on the CPU


def _optimise_setup(rays):
    """(start sigma, start coefficients, targets): the targets are field A's fp64 image; the start is A with sigma x 0.7 and
    coefficients x 0.8 plus noise"""
    sigma, co = lattice(2)
    target = R.march(sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP)[0].astype(np.float32)
    rng = np.random.default_rng(5)
    co0 = (co.astype(np.float32) * 0.8 + 0.05 * rng.standard_normal(co.shape)).astype(np.float16)
    return (sigma * np.float32(0.7)).astype(np.float32), co0, target


def test_it_optimises(tmp_path, rays):
    """40 full-batch steps at degree 2 on bricks of 8.  The NumPy reference optimiser (tests/baked_train_reference.py optimise, float64,
    on the dense arrays of the start field, run once on the CPU) brings the loss to REFERENCE_RATIO of its start; the GPU must reach at
    most twice that, the criterion of tests/test_gpu_baked_train.py test_it_optimises."""
    from keras_nerf_amd.baked import BakedField, BrickBakedField, load_field
    from keras_nerf_amd.baked_train import brick_optimizer
    sigma, co, target = _optimise_setup(rays)
    start = BakedField.from_arrays(sigma, co, (LO, HI)).compact(8)
    kept = start._records.clone()
    opt = brick_optimizer(start, *OPT_RATES, step=STEP)
    hist = opt.fit([(torch.as_tensor(target), (rays["o"], rays["d"], None))] * 40, rays["near"], rays["far"])["loss"]
    final = float(opt.accumulate(rays["o"], rays["d"], rays["near"], rays["far"], target))
    assert len(hist) == 40 and opt.iterations == 40
    ratio = final / hist[0]
    print(f"loss {hist[0]:.4e} -> {final:.4e}: ratio {ratio:.4e} (reference {REFERENCE_RATIO})")
    assert ratio <= 2.0 * REFERENCE_RATIO
    assert torch.equal(start._records, kept)                               # the field the optimiser was made from is untouched
    done = opt.finish()
    assert type(done) is BrickBakedField and done.sigma_threshold == start.sigma_threshold and done.brick == 8
    occ, sup = done.occupied.cpu().numpy(), opt.field.occupied.cpu().numpy()
    assert (occ <= sup).all() and np.array_equal(done.brick_of.cpu().numpy(), B.brick_table(occ, RES, 8)[0])
    done.save(tmp_path / "tuned.npz")
    back = load_field(tmp_path / "tuned.npz")
    assert type(back) is BrickBakedField and torch.equal(back._records, done._records)
    kw = dict(step=STEP, white_background=False)
    a, c, e = (f.render(rays["o"], rays["d"], rays["near"], rays["far"], **kw) for f in (done, back, opt.field))
    for key in OUT:
        assert torch.equal(a[key], c[key]) and torch.equal(a[key], e[key]), key
    from keras_nerf_amd.baked_bricks_train import brick_sigma
    cut = opt.finish(sigma_threshold=8.0)
    s, all_of_it = brick_sigma(cut)[1].cpu().numpy(), brick_sigma(done)[1].cpu().numpy()
    assert cut.sigma_threshold == 8.0 and ((s == 0) | (s > 8.0)).all() and (s == 0).sum() > (all_of_it == 0).sum() and s.any()
    assert np.array_equal(cut.occupied.cpu().numpy(), R.occupied_cells(s)) and cut.n_bricks <= done.n_bricks


def test_no_tensor_of_the_dense_table_is_made():
    """129^3 lattice, degree 2, one small blob: construction, one train_step and finish() together allocate less than the dense record
    table (129^3 x 64 bytes) above what was allocated before.  The dense optimiser cannot meet this: it clones the table."""
    from keras_nerf_amd.baked import BakedField, record_bytes
    from keras_nerf_amd.baked_train import brick_optimizer
    n, degree = 129, 2
    dev = torch.device("cuda")
    sigma = torch.zeros((n, n, n), device=dev)
    sigma[60:66, 58:64, 62:70] = 12.0
    co = torch.zeros((n, n, n, 9, 3), device=dev, dtype=torch.float16)
    co[..., 0, :] = 1.5
    field = BakedField.from_arrays(sigma, co, ((-1.0,) * 3, (1.0,) * 3)).compact(8)
    del sigma, co
    g = torch.Generator().manual_seed(3)
    o = torch.tensor([[0.0, 0.0, -3.0]]).repeat(64, 1)
    d = torch.nn.functional.normalize(torch.tensor([[0.0, 0.0, 3.0]]) + 0.05 * torch.randn((64, 3), generator=g), dim=1)
    o, d, target = o.to(dev), d.to(dev), torch.rand((64, 3), generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    opt = brick_optimizer(field, *RATES, dilation=1)
    loss = opt.train_step(o, d, 1.0, 5.0, target)
    done = opt.finish()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    table = n ** 3 * record_bytes(degree)
    print(f"peak {peak / 2 ** 20:.1f} MiB above the start; the dense table is {table / 2 ** 20:.1f} MiB; optimiser {opt.nbytes / 2 ** 20:.1f} MiB, "
          f"{opt.field.n_bricks} train bricks, {done.n_bricks} kept")
    assert 0 < peak < table
    assert float(loss) > 0 and np.isfinite(float(loss)) and 1 <= done.n_bricks <= opt.field.n_bricks < 100


def test_a_lane_count_the_degree_does_not_have_is_refused(rays):
    from keras_nerf_amd import _lib
    from keras_nerf_amd.baked import _stream
    from keras_nerf_amd.baked_train import brick_optimizer
    lib = _lib.load()
    for degree in (0, 1, 2, 3):
        r = _on_device(rays, degree)
        src = _source(degree, 8)
        opt = brick_optimizer(src, *RATES, step=STEP)
        sq = torch.full((N_RAYS,), -1.0, device=src.device)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        for lanes in (1, 2, 3, 4, 8):
            if lanes in BRICK_TRAIN_VARIANTS[degree]:
                continue
            with pytest.raises(ValueError, match="lanes_per_ray"):
                brick_optimizer(src, *RATES, step=STEP, lanes_per_ray=lanes)
            rc = lib.knerf_baked_bricks_train_rays(_stream(src.device), C.byref(opt._c), ptr(r["o"]), ptr(r["d"]), ptr(r["near"]),
                                                   ptr(r["far"]), 0.0, 0.0, ptr(r["target"]), N_RAYS, N_RAYS, STEP, 0.0,
                                                   _lib.BAKED_SKIP_EMPTY | (lanes << _lib.BAKED_LANES_SHIFT), ptr(sq))
            assert rc == _lib.KNERF_ERR_INVALID, (degree, lanes, rc)
        torch.cuda.synchronize()
        assert float(opt._grad.abs().max()) == 0.0 and bool((sq == -1.0).all())          # nothing was launched
        for lanes in BRICK_TRAIN_VARIANTS[degree]:                                        # and the ones that exist run
            assert float(brick_optimizer(src, *RATES, step=STEP, lanes_per_ray=lanes).accumulate(*_batch(r))) > 0
