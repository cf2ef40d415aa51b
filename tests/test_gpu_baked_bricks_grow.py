"""Growing a brick baked field on the GPU (keras_nerf_amd/baked_bricks_grow.py, csrc/baked_bricks_grow.hip): resampling byte for byte
against the NumPy mirror and against the dense path, its memory condition, the regulariser against fp64 and bit for bit against the dense
launch, the one deterministic add, the support invariant with TV on and across a prune, what a prune builds and carries, a coarse-to-fine
fit, and the refusals on live buffers.  Tolerances and measured values: tests/README_baked_bricks_grow.md.  No element is left out of
any comparison.  No test feeds a kernel a damaged table or key: the range guards are checked by reading."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import baked_bricks_grow_reference as W
from tests import baked_bricks_train_reference as S
from tests import baked_grow_reference as G
from tests.test_baked_bricks_grow_host import BRICKS, DESTINATIONS, HI, LO, RES, THRESHOLDS, lattice, three_blobs
from tests.test_gpu_baked import N_RAYS, STEP, rays  # noqa: F401 -- the ray set of the dense render tests (a fixture), over the same box

pytestmark = pytest.mark.gpu

TV = dict(tv_sigma=2e-2, tv_sh=5e-2, tv_epsilon=1e-6)
RATES = (0.05, 0.01)
U = 2.0 ** -24
OUT = ("image", "depth", "opacity")

_fields, _device_rays = {}, {}


def _source(degree, b, blobs=2):
    """the brick field of the test lattice, built once and never changed (a trainer works on a copy, a resample writes a new field)"""
    from keras_nerf_amd.baked import BakedField
    key = (degree, b, blobs)
    if key not in _fields:
        sigma, co = (lattice if blobs == 2 else three_blobs)(degree)
        _fields[key] = BakedField.from_arrays(sigma, co, (LO, HI)).compact(b)
    return _fields[key]


def _on_device(rays):
    if not _device_rays:
        target = np.random.default_rng(42).uniform(0.0, 1.0, (N_RAYS, 3)).astype(np.float32)
        _device_rays.update({k: torch.as_tensor(v).cuda() for k, v in {**rays, "target": target}.items()})
    return _device_rays


def _batch(r):
    return r["o"], r["d"], r["near"], r["far"], r["target"]


def _words(cells):
    from keras_nerf_amd.runtime import pack_occupancy
    return pack_occupancy(cells).view(np.int32)


def _same_field(got, records, brick_of, n, cells, what):
    assert got.n_bricks == n, what
    assert np.array_equal(got.brick_of.cpu().numpy(), brick_of), what
    assert np.array_equal(got._words.cpu().numpy(), _words(cells)), what
    assert np.array_equal(got._records.cpu().numpy(), records), what


def _skip_is_exact(field, r):
    a = field.render(r["o"], r["d"], r["near"], r["far"], step=STEP, skip_empty=True)
    b = field.render(r["o"], r["d"], r["near"], r["far"], step=STEP, skip_empty=False)
    for key in OUT:
        assert torch.equal(a[key], b[key]), key
    return a


# ---- resampling

@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_resample_is_the_mirror_byte_for_byte(degree, b, rays):
    from keras_nerf_amd import _lib
    from keras_nerf_amd.baked import BrickBakedField, _stream
    from keras_nerf_amd.baked_bricks_grow import resample_bricks
    from keras_nerf_amd.runtime import _ptr
    src = _source(degree, b)
    before = src._records.clone()
    bricks, brick_of = src._records.cpu().numpy(), src.brick_of.cpu().numpy()
    assert (brick_of < 0).any() and src.n_bricks == {4: 16, 8: 11}[b]
    r = _on_device(rays)
    for res in DESTINATIONS:
        for thr in THRESHOLDS:
            what = (res, thr)
            sigma, cells, want_of, n, want = W.resample(bricks, brick_of, RES, b, res, degree, thr)
            got = resample_bricks(src, res, thr)
            assert type(got) is BrickBakedField and got.resolution == res and got.brick == b and got.sigma_threshold == thr
            assert got.sh_degree == degree and got.bounds == src.bounds
            _same_field(got, want, want_of, n, cells, what)
            if res == (2, 2, 2):
                assert n == 1 and not want.any() and (want_of == -1).all()                     # the one all-zero brick
            else:
                assert cells.any() and bool((want_of < 0).any()) == (res != (10, 9, 7) or b == 4)   # (the coarser lattice at b = 8: 2 x 2 x 1 bricks, all stored)
            # the sigma pass alone: the mirror's sigma bit for bit
            out = torch.full(res, -1.0, device=src.device)
            assert _lib.load().knerf_baked_resample_bricks_sigma(_stream(src.device), C.byref(src._c), (C.c_int32 * 3)(*res), thr, _ptr(out)) == 0
            assert np.array_equal(out.cpu().numpy().view(np.int32), sigma.view(np.int32)), what
            # the dense path gives the same field
            dense = src.to_dense().resample(res, thr).compact(b)
            _same_field(dense, want, want_of, n, cells, what)
            if thr == 0.0:
                image = _skip_is_exact(got, r)["image"]
                assert res == (2, 2, 2) or float(image.abs().max()) > 0
    assert torch.equal(src._records, before)                                                   # the source is left as it is


@pytest.mark.parametrize("b,b_new", [(4, 8), (8, 4)])
def test_resample_onto_another_brick_size(b, b_new):
    from keras_nerf_amd.baked_bricks_grow import resample_bricks
    src = _source(2, b)
    bricks, brick_of = src._records.cpu().numpy(), src.brick_of.cpu().numpy()
    for res, thr in (((37, 33, 23), 0.0), ((23, 7, 40), 10.0)):
        _, cells, want_of, n, want = W.resample(bricks, brick_of, RES, b, res, 2, thr, b_new)
        got = resample_bricks(src, res, thr, brick=b_new)
        assert got.brick == b_new
        _same_field(got, want, want_of, n, cells, (res, thr))


def test_resample_forms_no_dense_table():
    """65^3 -> 129^3 at degree 2 from a blob: the peak allocation stays below the dense destination table's 129^3 x 64 bytes"""
    from keras_nerf_amd.baked import BakedField
    from keras_nerf_amd.baked_bricks_grow import resample_bricks
    R0, R1 = 65, 129
    rng = np.random.default_rng(3)
    x, y, z = np.meshgrid(*(np.arange(R0, dtype=np.float32),) * 3, indexing="ij")
    inside = (x - 30) ** 2 + (y - 34) ** 2 + (z - 28) ** 2 < 13.0 ** 2
    sigma = np.where(inside, rng.uniform(5.0, 30.0, (R0,) * 3), 0.0).astype(np.float32)
    co = (rng.standard_normal((R0,) * 3 + (9, 3)) * 0.4).astype(np.float16)
    src = BakedField.from_arrays(sigma, co, (LO, HI)).compact(8)
    share = float(src.occupied.float().mean())
    assert 0.0 < share < 0.10
    del sigma, co
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    out = resample_bricks(src, R1)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - start
    table = R1 ** 3 * 64
    print(f"occupied cells {share:.3f}; peak {peak / 2 ** 20:.1f} MiB above the start, dense destination table {table / 2 ** 20:.1f} MiB; "
          f"{out.n_bricks} of {17 ** 3} bricks stored ({out.nbytes / 2 ** 20:.1f} MiB)")
    assert peak < table
    assert out.resolution == (R1,) * 3 and 1 < out.n_bricks < 17 ** 3 // 4 and float(out.occupied.float().mean()) < 0.10


# ---- the regulariser

def _structure(flags, brick_of, b):
    """what the slot set of a trainer has, from its flags and brick table (NumPy)"""
    has = (W.slot_of_rows(brick_of, flags, RES, b) >= 0).reshape(RES)
    at = S.row_points(brick_of, RES, b)
    train = np.zeros(int(np.prod(RES)), dtype=bool)
    train[at[(at >= 0) & ((flags & 2) != 0)]] = True
    x, y, z = np.meshgrid(*(np.arange(n) for n in RES), indexing="ij")
    stored = brick_of[x // b, y // b, z // b] >= 0
    out = {"beside": False, "absent": False, "across": [False] * 3, "face": False, "fixed": bool((has & ~train.reshape(RES)).any())}
    for p in np.argwhere(has):
        for a in range(3):
            for s in (-1, 1):
                q = p.copy()
                q[a] += s
                if q[a] < 0 or q[a] >= RES[a]:
                    out["face"] = True
                    continue
                same = bool((q // b == p // b).all())
                out["beside"] |= same and not has[tuple(q)]
                out["absent"] |= not stored[tuple(q)]
                out["across"][a] |= (not same) and bool(has[tuple(q)])
    return out, has, train.reshape(RES)


def _tv_setup(degree, b, dilation, **tv):
    """a trainer over the three blobs whose master rows of slots are perturbed by noise (the sigma of a slot that is not trainable stays
    0, rows of records that are no slot stay zero); (trainer, master fp32 rows, flags, brick_of)"""
    from keras_nerf_amd.baked_bricks_grow import grid_trainer
    tr = grid_trainer(_source(degree, b, 3), *RATES, step=STEP, dilation=dilation, **{**TV, **tv})
    flags, brick_of = tr._flags.cpu().numpy(), tr.field.brick_of.cpu().numpy()
    slot, train = (flags & 1) != 0, (flags & 2) != 0
    rng = np.random.default_rng(11 + degree)
    m = tr._master.cpu().numpy().astype(np.float64)
    assert m[~slot].any() and not m[~train, 0].any()                       # (a record that is no slot has a master row too: its coefficients)
    noise = rng.normal(0.0, 0.2, m.shape)
    noise[:, 0] = np.abs(noise[:, 0]) * 3.0
    noise[~slot] = 0                                                       # those rows stay as they are: no launch may look at them
    m = (m + noise).astype(np.float32)
    m[~train, 0] = 0
    tr._master.copy_(torch.as_tensor(m))
    return tr, m, flags, brick_of


def _weights(tr):
    """the per-term weights as the launch receives them: formed in double, passed as float32"""
    ws, wc = tr.tv_weights()
    return float(np.float32(ws)), float(np.float32(wc))


@pytest.mark.parametrize("dilation", [0, 1])
@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_tv_matches_fp64_and_the_dense_launch(degree, b, dilation):
    tr, m, flags, brick_of = _tv_setup(degree, b, dilation)
    K = (degree + 1) ** 2
    slot = (flags & 1) != 0
    have, has, train = _structure(flags, brick_of, b)
    # slots beside records that are none inside a stored brick, neighbours across brick faces on all three axes, slots on lattice faces,
    # sigma that is not trainable; a neighbour in an absent brick in every case but one (b = 8 with dilation 1: the grown support of the
    # third blob ends inside its bricks there)
    assert have["beside"] and all(have["across"]) and have["face"] and have["fixed"] and have["absent"] == ((b, dilation) != (8, 1))
    assert tr.n_slots == int(slot.sum()) == int(has.sum()) and slot.sum() < slot.size
    ws, wc = _weights(tr)
    assert ws == pytest.approx(TV["tv_sigma"] / tr.n_slots, rel=1e-7) and wc == pytest.approx(TV["tv_sh"] / (3 * K * tr.n_slots), rel=1e-7)
    value, grad, sums = W.tv_value_and_grad(m.astype(np.float64), brick_of, flags, RES, b, ws, wc, float(np.float32(TV["tv_epsilon"])))
    # the rows that are no slot are prefilled: they must keep their bits
    fill = torch.zeros_like(tr._grad)
    fill[torch.as_tensor(~slot).to(fill.device)] = -0.0
    fill[torch.as_tensor(~slot).to(fill.device), 0] = 0.375
    tr._grad.copy_(fill)
    tv_s, tv_c = tr.regularize()
    assert tv_s.dtype == torch.float64 and tv_s.dim() == 0 and tv_c.dtype == torch.float64 and tv_c.is_cuda
    got = tr._grad.cpu().numpy()
    assert np.array_equal(got[~slot].view(np.int32), fill.cpu().numpy()[~slot].view(np.int32))          # exactly untouched
    err_s, err_c = float(np.abs(got[slot, 0] - grad[slot, 0]).max()), float(np.abs(got[slot, 1:] - grad[slot, 1:]).max())
    want = (sums[0] / tr.n_slots, sums[1] / (3 * K * tr.n_slots))
    rel = (abs(float(tv_s) - want[0]) / want[0], abs(float(tv_c) - want[1]) / want[1])
    print(f"degree {degree} b {b} dilation {dilation}: max |g - fp64| / w: sigma {err_s / ws / U:.2f} x 2^-24, coefficients "
          f"{err_c / wc / U:.2f} x 2^-24 (bound 64 x 2^-24); value: relative error {rel[0]:.2e} (sigma), {rel[1]:.2e} (coefficients)")
    assert np.abs(grad[slot, 0]).max() > ws and np.abs(grad[slot, 1:]).max() > wc                    # the gradient is there
    assert not grad[~slot].any()
    assert err_s <= 64 * U * ws and err_c <= 64 * U * wc
    assert rel[0] <= 1e-6 and rel[1] <= 1e-6
    # the dense optimiser of to_dense(), fed the same master values and a zero gradient: the same bits in every row of a slot
    dense = _source(degree, b, 3).to_dense().optimizer(*RATES, step=STEP, dilation=dilation, **TV)
    assert dense.n_slots == tr.n_slots and torch.equal(dense.slot_mask, tr.slot_mask)
    rows = tr._dense(tr._master, torch.float32)[dense._index]
    dense._master.copy_(rows)
    prefill = torch.as_tensor(np.random.default_rng(degree).normal(0.0, 1e-4, tuple(dense._grad.shape)).astype(np.float32)).cuda()
    dense._grad.copy_(prefill)
    tr._grad.zero_()
    at = torch.as_tensor(W.slot_of_rows(brick_of, flags, RES, b)).cuda()[dense._index]                 # the row of every dense slot
    tr._grad[at] = prefill
    d_s, d_c = dense.regularize()
    b_s, b_c = tr.regularize()
    assert torch.equal(tr._grad[at].view(torch.int32), dense._grad.view(torch.int32))
    assert float(tr._grad[torch.as_tensor(~slot).cuda()].abs().max()) == 0.0
    assert abs(float(d_s) - float(b_s)) <= 1e-12 * abs(float(d_s)) and abs(float(d_c) - float(b_c)) <= 1e-12 * abs(float(d_c))


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 2, 3])
def test_tv_is_one_deterministic_add(degree, b):
    tr, _, flags, _ = _tv_setup(degree, b, 1)
    slot = torch.as_tensor((flags & 1) != 0).cuda()
    tr.regularize()
    alone = tr._grad.clone()
    assert float(alone.abs().max()) > 0 and float(alone[~slot].abs().max()) == 0
    rng = np.random.default_rng(5)
    before = torch.as_tensor(rng.normal(0.0, 1e-4, tuple(alone.shape)).astype(np.float32)).to(alone.device)
    before[::7] = -0.0
    runs = []
    for _ in range(2):
        tr._grad.copy_(before)
        tv = tr.regularize()
        runs.append((tr._grad.clone(), tv))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))                  # two runs: the same bits
    assert torch.equal(runs[0][1][0], runs[1][1][0]) and torch.equal(runs[0][1][1], runs[1][1][1])
    want = before.cpu().numpy() + alone.cpu().numpy()                                               # fp32(before + g), one rounding
    want[~slot.cpu().numpy()] = before.cpu().numpy()[~slot.cpu().numpy()]                           # (a record that is no slot: not even + 0)
    assert np.array_equal(runs[0][0].cpu().numpy().view(np.int32), want.view(np.int32))
    # a weight of exactly 0 leaves the columns of its group untouched, bit for bit (the prefill holds -0.0, which an added +0 would flip)
    for off, cols, rest in (("tv_sigma", slice(0, 1), slice(1, None)), ("tv_sh", slice(1, None), slice(0, 1))):
        saved = getattr(tr, off)
        setattr(tr, off, 0.0)
        tr._grad.copy_(before)
        both = tr.regularize()
        setattr(tr, off, saved)
        after = tr._grad
        assert torch.equal(after[:, cols].view(torch.int32), before[:, cols].view(torch.int32)), off
        assert torch.equal(after[:, rest].view(torch.int32), runs[0][0][:, rest].view(torch.int32)), off
        assert torch.equal(both[0], runs[0][1][0]) and torch.equal(both[1], runs[0][1][1])          # the values are reported all the same


def test_both_weights_zero_is_the_plain_brick_optimiser(rays):
    """no further launch: the records after three steps are BrickFieldOptimizer's, and fit's dict has no tv entries"""
    from keras_nerf_amd.baked_bricks_grow import grid_trainer
    from keras_nerf_amd.baked_train import brick_optimizer
    r = _on_device(rays)
    src = _source(2, 8, 3)
    tr, plain = grid_trainer(src, *RATES, step=STEP), brick_optimizer(src, *RATES, step=STEP)
    assert not tr.regularized and tr.last_regularizer is None
    called = []
    tr.regularize = lambda: called.append(1)
    batches = [(r["target"][:1], (r["o"][:1], r["d"][:1], None))] * 3            # one ray per launch: the sums do not depend on arrival order
    hist = tr.fit(batches, r["near"][:1], r["far"][:1])
    plain.fit(batches, r["near"][:1], r["far"][:1])
    assert sorted(hist) == ["loss"] and len(hist["loss"]) == 3 and not called
    assert torch.equal(tr.field._records, plain.field._records) and torch.equal(tr._m, plain._m)


@pytest.mark.parametrize("dilation", [0, 1])
def test_nothing_leaves_the_support_with_tv_on_and_across_a_prune(dilation, rays):
    """20 regularised steps at a sigma rate of 2 with a prune after the tenth: a render with and without skipping gives the same bits
    after every step"""
    from keras_nerf_amd.baked_bricks_grow import grid_trainer
    r = _on_device(rays)
    tr = grid_trainer(_source(2, 8, 3), 2.0, 0.05, step=STEP, dilation=dilation, **TV)
    losses = []
    for k in range(20):
        if k == 10:
            info = tr.prune(1.0)
            # (with a dilation the support is grown again around what sigma has become: only without one the counts cannot grow)
            assert (info["after"]["n_slots"] <= info["before"]["n_slots"] or dilation) and tr.iterations == 10
            _skip_is_exact(tr.field, r)
        losses.append(tr.train_step(*_batch(r)))
        _skip_is_exact(tr.field, r)
    assert tr.iterations == 20 and tr.last_regularizer is not None
    flags = tr._flags
    sigma = tr.field._records.reshape(-1, tr.field._records.shape[2])[:, :4].contiguous().view(torch.float32).reshape(-1)
    assert bool((sigma[(flags & 2) == 0] == 0).all()) and bool((sigma >= 0).all()) and bool(torch.isfinite(sigma).all())
    assert bool((tr._master[(flags & 2) == 0, 0] == 0).all())                                      # the master of a fixed sigma stays 0
    assert all(np.isfinite(float(v)) for v in losses)


# ---- prune

@pytest.mark.parametrize("dilation", [0, 1])
@pytest.mark.parametrize("b", BRICKS)
def test_prune_builds_the_trainer_of_the_finished_field_and_carries_the_state(b, dilation, rays):
    from keras_nerf_amd.baked_bricks_grow import grid_trainer
    r = _on_device(rays)
    degree, thr = 2, 7.5
    kw = dict(step=STEP, dilation=dilation, **TV)
    tr = grid_trainer(_source(degree, b, 3), *RATES, **kw)
    for _ in range(3):
        tr.train_step(*_batch(r))
    tr.accumulate(*_batch(r))                                               # a pending gradient: the prune discards it
    old = {k: getattr(tr, k).cpu().numpy().copy() for k in ("_master", "_m", "_v", "_flags")}
    old_of = tr.field.brick_of.cpu().numpy().copy()
    assert np.abs(old["_m"]).max() > 0 and np.abs(old["_v"]).max() > 0 and float(tr._grad.abs().max()) > 0
    want = grid_trainer(tr.finish(thr), *RATES, **kw)
    info = tr.prune(thr)
    assert info["before"]["n_bricks"] == old_of.max() + 1 and info["after"] == tr.counts() == want.counts()
    # the third blob is gone, and with it a brick, unless it shares its only brick with the first blob (b = 8 without dilation)
    assert info["after"]["n_slots"] < info["before"]["n_slots"]
    assert (info["after"]["n_bricks"] < info["before"]["n_bricks"]) or ((b, dilation) == (8, 0) and info["after"]["n_bricks"] <= 11)
    assert info["after"]["n_records"] == info["after"]["n_bricks"] * b ** 3
    # the live field, the flags and the support are those of a trainer built on the finished field
    for name in ("_records", "_brick_of", "_words"):
        assert torch.equal(getattr(tr.field, name), getattr(want.field, name)), name
    assert torch.equal(tr._flags, want._flags) and tr.n_slots == want.n_slots and tr.field.n_bricks == want.field.n_bricks
    assert torch.equal(tr._keys, want._keys) and tr.field.sigma_threshold == want.field.sigma_threshold
    assert tr.iterations == 3 and tr.dilation == dilation and float(tr._grad.abs().max()) == 0.0
    # what is carried and what starts at zero
    new_of, new_flags = tr.field.brick_of.cpu().numpy(), tr._flags.cpu().numpy()
    row, sig = W.carried_rows(old_of, old["_flags"], new_of, new_flags, RES, b)
    kept = row >= 0
    assert kept.any() and sig.any() and (kept & ~sig).any() and (~kept).any()
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    for name in ("_master", "_m", "_v"):
        now = getattr(tr, name).cpu().numpy()
        assert np.array_equal(bits(now[kept, 1:]), bits(old[name][row[kept], 1:])), name
        if name != "_master":
            assert np.array_equal(bits(now[sig, 0]), bits(old[name][row[sig], 0])), name
            assert not now[~kept].any() and not now[~sig, 0].any(), name
    assert torch.equal(tr._master[:, 0], want._master[:, 0])               # master sigma is the new record's sigma
    assert np.array_equal(bits(tr._master.cpu().numpy()[~kept]), bits(want._master.cpu().numpy()[~kept]))
    # fp16(master) is the record's coefficients at every slot
    K = (degree + 1) ** 2
    rec = tr.field._records.reshape(-1, tr.field._records.shape[2])
    coef = rec[:, 4:4 + 6 * K].contiguous().view(torch.float16)
    slot = (tr._flags & 1) != 0
    assert torch.equal(tr._master[slot, 1:].to(torch.float16).view(torch.int16), coef[slot].view(torch.int16))
    assert torch.equal(tr._master[slot, 0], rec[:, :4].contiguous().view(torch.float32).reshape(-1)[slot] * ((tr._flags[slot] & 2) != 0))
    # and it trains on
    before = tr.field._records.clone()
    loss = tr.train_step(*_batch(r))
    assert tr.iterations == 4 and np.isfinite(float(loss)) and not torch.equal(tr.field._records, before)
    _skip_is_exact(tr.field, r)
    # nothing left to optimise: refused, and the trainer stays as it is
    state = tr._master.clone()
    with pytest.raises(ValueError, match="nothing to optimise"):
        tr.prune(1e9)
    assert torch.equal(tr._master, state) and tr.iterations == 4


# ---- coarse to fine

def test_coarse_to_fine_on_bricks(tmp_path):
    """the lattice, rays, schedule and criterion of tests/test_gpu_baked_grow.py test_coarse_to_fine, started from the compacted field"""
    from keras_nerf_amd.baked import BrickBakedField
    from keras_nerf_amd.baked_bricks_grow import fit_coarse_to_fine_bricks
    from tests import test_gpu_baked_grow as D
    sa, ca, rays_, target = D._c2f_setup()
    sigma, co = D._lattice(2)
    start = D._field(sigma * np.float32(0.7), co).compact(4)
    kept = start._records.clone()
    batches = iter([(target, (rays_["o"], rays_["d"], None))] * 45)
    kw = dict(learning_rate_sigma=D.C2F_RATES[0], learning_rate_sh=D.C2F_RATES[1], step=D.STEP, **D.C2F)
    done, hist = fit_coarse_to_fine_bricks(start, batches, rays_["near"], rays_["far"], D.C2F_STAGES, **kw)
    assert len(list(batches)) == 5                                                                  # 40 batches were consumed, none dropped
    assert type(done) is BrickBakedField and done.resolution == D.FINE and done.brick == 4
    assert len(hist["loss"]) == 40 and len(hist["tv_sigma"]) == 40 and len(hist["tv_sh"]) == 40
    assert [s["resolution"] for s in hist["stages"]] == [D.RES, D.FINE] and [s["steps"] for s in hist["stages"]] == [20, 20]
    for s in hist["stages"]:
        assert s["prunes"] == [] and 0 < s["n_slots"] <= s["n_records"] == s["n_bricks"] * 64
    assert hist["stages"][1]["n_slots"] > hist["stages"][0]["n_slots"]
    img = done.render(rays_["o"], rays_["d"], rays_["near"], rays_["far"], step=D.STEP, outputs="image")["image"]
    final = float(((img - torch.as_tensor(target).to(img.device)).to(torch.float64) ** 2).mean())
    ratio = final / hist["loss"][0]
    ref = D._reference_ratio(sa, ca, rays_, target)
    print(f"loss {hist['loss'][0]:.4e} -> {final:.4e}: ratio {ratio:.4e} (NumPy loop on the dense arrays {ref[0]:.4e} -> {ref[1]:.4e}: ratio "
          f"{ref[2]:.4e})")
    assert ref[2] < 0.05                                                                            # the loop does optimise
    assert ratio <= 2.0 * ref[2]
    assert torch.equal(start._records, kept)                                                        # the start is untouched
    # pruning while fitting: structure only
    batches = iter([(target, (rays_["o"], rays_["d"], None))] * 45)
    pruned, hist = fit_coarse_to_fine_bricks(start, batches, rays_["near"], rays_["far"], D.C2F_STAGES, sigma_threshold=0.3, prune_every=6, **kw)
    assert len(list(batches)) == 5 and len(hist["loss"]) == 40 and pruned.sigma_threshold == 0.3 and pruned.resolution == D.FINE
    for s in hist["stages"]:
        assert len(s["prunes"]) == 3                                                                # after steps 6, 12, 18 of 20
        chain = [s["prunes"][0]["before"]] + [p["after"] for p in s["prunes"]]
        for a, c in zip(chain, chain[1:]):
            assert all(c[k] <= a[k] for k in ("n_bricks", "n_records", "n_slots")), (a, c)        # dilation 0: counts never grow
        assert [p["before"] for p in s["prunes"][1:]] == [p["after"] for p in s["prunes"][:-1]]
        assert {k: s[k] for k in ("n_bricks", "n_records", "n_slots")} == s["prunes"][-1]["after"]
    pruned.save(tmp_path / "grown.npz")
    back = BrickBakedField.load(tmp_path / "grown.npz")
    assert torch.equal(back._records, pruned._records) and torch.equal(back.brick_of, pruned.brick_of)
    a = pruned.render(rays_["o"], rays_["d"], rays_["near"], rays_["far"], step=D.STEP)
    c = pruned.render(rays_["o"], rays_["d"], rays_["near"], rays_["far"], step=D.STEP, skip_empty=False)
    for key in OUT:
        assert torch.equal(a[key], c[key]), key


# ---- refusals on live buffers

def test_refusals_leave_the_destinations_as_they_were():
    from keras_nerf_amd import _lib
    from keras_nerf_amd.baked import _stream
    from keras_nerf_amd.baked_bricks_grow import grid_trainer, resample_bricks, stored_keys
    from keras_nerf_amd.runtime import _ptr
    lib, INV = _lib.load(), _lib.KNERF_ERR_INVALID
    src = _source(1, 8)
    dev = src.device
    tr = grid_trainer(src, *RATES, **TV)
    tr._grad.fill_(0.25)
    tv = torch.full((int(tr._flags.numel()), 2), -3.0, device=dev)
    call = lambda c=None, keys=tr._keys, flags=tr._flags, master=tr._master, ws=1e-3, wc=1e-3, eps=1e-6: lib.knerf_baked_bricks_train_tv(
        _stream(dev), C.byref(c if c is not None else tr._c), _ptr(keys), _ptr(flags), _ptr(master), ws, wc, eps, _ptr(tv))
    f = tr.field
    too_many = _lib.KnerfBakedBricks(C.c_void_p(f._records.data_ptr()), C.c_void_p(f._brick_of.data_ptr()), C.c_void_p(f._words.data_ptr()),
                                     (C.c_int32 * 3)(*RES), 1, (C.c_float * 3)(*LO), (C.c_float * 3)(*HI), 3, 19)
    broken = _lib.KnerfBakedBricksTrain(too_many, C.c_void_p(tr._grad.data_ptr()))
    no_grad = _lib.KnerfBakedBricksTrain(f._c, None)
    for bad in (dict(keys=None), dict(flags=None), dict(master=None), dict(ws=-1e-3), dict(wc=float("nan")), dict(ws=float("inf")),
                dict(eps=0.0), dict(eps=float("nan")), dict(eps=-1e-6), dict(c=broken), dict(c=no_grad)):
        assert call(**bad) == INV, bad
    torch.cuda.synchronize()
    assert bool((tr._grad == 0.25).all()) and bool((tv == -3.0).all())
    assert call() == 0                                                                              # and the good call does write
    torch.cuda.synchronize()
    assert not bool((tr._grad == 0.25).all()) and not bool((tv == -3.0).any())
    # the two passes of a resample
    res = (37, 33, 23)
    good = resample_bricks(src, res)
    sig = torch.full(res, -2.0, device=dev)
    rec = torch.full_like(good._records, 0xAB)
    keys = stored_keys(good._brick_of)
    sigma = lambda s=src._c, new=res, thr=0.0, out=sig: lib.knerf_baked_resample_bricks_sigma(_stream(dev), C.byref(s), (C.c_int32 * 3)(*new),
                                                                                               thr, _ptr(out))
    records = lambda s=src._c, d=good._c, k=keys, thr=0.0, out=rec: lib.knerf_baked_resample_bricks(_stream(dev), C.byref(s), C.byref(d),
                                                                                                     _ptr(k), thr, _ptr(out))
    wrong = _lib.KnerfBakedBricks(C.c_void_p(src._records.data_ptr()), C.c_void_p(src._brick_of.data_ptr()), None, (C.c_int32 * 3)(*RES), 5,
                                  (C.c_float * 3)(*LO), (C.c_float * 3)(*HI), 3, src.n_bricks)
    other_box = _lib.KnerfBakedBricks(None, C.c_void_p(good._brick_of.data_ptr()), None, (C.c_int32 * 3)(*res), 1, (C.c_float * 3)(*LO),
                                      (C.c_float * 3)(1.0, 0.8, 0.75), 3, good.n_bricks)
    inside = _lib.KnerfBakedBricks(C.c_void_p(rec[1:].data_ptr()), C.c_void_p(src._brick_of.data_ptr()), None, (C.c_int32 * 3)(*RES), 1,
                                   (C.c_float * 3)(*LO), (C.c_float * 3)(*HI), 3, src.n_bricks)             # a source inside the destination
    for bad in (dict(new=(1, 33, 23)), dict(new=(37, 33, 1026)), dict(thr=-1.0), dict(thr=float("nan")), dict(out=None), dict(s=wrong)):
        assert sigma(**bad) == INV, bad
    for bad in (dict(thr=-1.0), dict(thr=float("inf")), dict(out=None), dict(k=None), dict(s=wrong), dict(d=other_box), dict(s=inside)):
        assert records(**bad) == INV, bad
    torch.cuda.synchronize()
    assert bool((sig == -2.0).all()) and bool((rec == 0xAB).all())
    assert sigma() == 0 and records() == 0                                                          # and the good calls do write
    assert torch.equal(rec, good._records) and not bool((sig == -2.0).any())
