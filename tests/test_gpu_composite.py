"""csrc/composite.hip's training half -- MSE, clip gate, dL/d(rgb, sigma) with its mirrored wave scan, dead-tile flags, list append --
and compact_tiles_kernel on caller-made inputs (knerf_debug_composite_train / knerf_debug_compact_tiles) against the float64
reference of tests/composite_reference.py.  Cases, ray classes and tolerances are that module's; tests/test_composite_host.py
proves on the CPU what the tolerances rest on (tol = 8 x the float32 mirror's error, from NumPy alone) and that every mutant of the
reference is far outside them.  Each test prints its figures before it asserts (pytest -s).

"Exactly zero" below means `== 0` for every element: where the gradient of a ray is gated off the kernel forms 0 * rgb and sums
of such products, whose sign bit follows rgb -- a -0.0 is as dead for the backward chain as a +0.0, and the kernel's own dead rule
compares with == as well.

Measured on an MI355X, worst over the 36 cases (device error / tol): see tests/README.md.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import composite_reference as CR

pytestmark = pytest.mark.gpu

_CACHE = {}


def _p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _forward(raw, t, white):
    """knerf_composite of the product ABI: image, depth, weights"""
    from keras_nerf_amd import _lib
    R, S = t.shape
    img, dep, w = torch.empty((R, 3), device=raw.device), torch.empty((R,), device=raw.device), torch.empty((R, S), device=raw.device)
    stream = C.c_void_p(torch.cuda.current_stream(raw.device).cuda_stream)
    assert _lib.load().knerf_composite(stream, _p(raw), _p(t), R, S, int(white), _p(img), _p(dep), _p(w)) == 0
    return img, dep, w


def device_inputs(S, white):
    """the case's inputs on the device; rays of class OWN_PIXEL get the bits of their own forward pixel as target"""
    key = ("in", S, white)
    if key not in _CACHE:
        c = CR.case(S, white)
        raw, t = torch.from_numpy(c["raw"].copy()).cuda(), torch.from_numpy(c["t"].copy()).cuda()
        fwd = _forward(raw, t, white)
        target = torch.from_numpy(c["target"].copy()).cuda()
        own = torch.from_numpy(c["own"].copy()).cuda()
        target[own] = fwd[0][own]
        _CACHE[key] = (c, raw, t, target.contiguous(), fwd)
    return _CACHE[key]


def train(S, white, **kw):
    from keras_nerf_amd import debug
    c, raw, t, target, _ = device_inputs(S, white)
    out = debug.composite_train(raw, t, target, white, c["grad_scale"], c["loss_scale"], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def default_run(S, white):
    key = ("out", S, white)
    if key not in _CACHE:
        _CACHE[key] = train(S, white, loss0=CR.LOSS0)
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("S,white", CR.CASES)
def test_values_against_fp64(S, white):
    c = CR.case(S, white)
    out, ref, tol, skip = default_run(S, white), c["ref"], c["tol"], c["skip"]
    e = CR.errors(dict(out, loss=float(out["loss"][0])), ref, skip)
    print(f"\nS {S:4d} white {white}: " + "  ".join(f"{k} {e[k]:.2e}/{tol[k]:.2e}={e[k] / tol[k]:.2f}" for k in e))
    for k in ("image", "depth", "weights", "draw", "last", "loss"):
        assert e[k] <= tol[k], (k, e[k], tol[k])
    # a ray whose reference draw is all zero is all zero on the device (classes 7 and 8 at least), undecidable or not
    zero = ~np.abs(ref["draw"]).reshape(len(skip), -1).any(axis=1)
    assert zero[np.isin(c["cls"], (CR.RGB_OUTSIDE, CR.OWN_PIXEL))].all()
    assert (out["draw"][zero] == 0).all()
    # all sigma zero: the gate is open on pre == 0 / pre == 1 exactly; no weight, but dsigma = dw delta != 0 on every sample
    z = c["cls"] == CR.ALL_ZERO
    assert (out["draw"][z, :, :3] == 0).all() and (out["draw"][z, :, 3] != 0).all() and not out["weights"][z].any()
    assert (CR.last_mask(ref, skip).sum() >= 0.3 * len(skip))             # the last sample's own comparison is not empty
    assert np.isfinite(out["draw"]).all()


@pytest.mark.parametrize("S,white", CR.CASES)
def test_training_call_equals_forward_call_bit_for_bit(S, white):
    _, _, _, _, fwd = device_inputs(S, white)
    out = default_run(S, white)
    for got, want in zip((out["image"], out["depth"], out["weights"]), fwd):
        assert np.array_equal(bits(got), bits(want.cpu().numpy()))


@pytest.mark.parametrize("S,white", [(5, 0), (64, 1), (192, 0), (513, 1), (1024, 0)])
def test_loss_forms(S, white):
    """atomic form: added onto a non-zero start, within tol of the float64 sum (test_values_against_fp64 checks every case); the
    loss_partial form: within tol as well, and bit-identical over two calls, per-workgroup terms included"""
    c = CR.case(S, white)
    a = default_run(S, white)
    zero_start = train(S, white, loss0=0.0)
    assert abs(float(a["loss"][0]) - c["ref"]["loss"]) <= c["tol"]["loss"]
    assert abs(float(zero_start["loss"][0]) - (c["ref"]["loss"] - CR.LOSS0)) <= c["tol"]["loss"]
    assert float(a["loss"][0]) > CR.LOSS0 + 10 * c["tol"]["loss"]                  # the chunk's term is not lost in the start value
    p1, p2 = train(S, white, loss0=CR.LOSS0, partial=True), train(S, white, loss0=CR.LOSS0, partial=True)
    assert np.array_equal(bits(p1["loss"]), bits(p2["loss"])) and np.array_equal(bits(p1["loss_partial"]), bits(p2["loss_partial"]))
    print(f"\nS {S} white {white}: loss atomic {a['loss'][0]!r} partial {p1['loss'][0]!r} fp64 {c['ref']['loss']!r} tol {c['tol']['loss']:.2e}")
    assert abs(float(p1["loss"][0]) - c["ref"]["loss"]) <= c["tol"]["loss"]
    rp = CR.ref_partials(c["ref"]["image"], c["target"], c["own"], c["loss_scale"])
    assert p1["loss_partial"].shape == rp.shape and np.abs(p1["loss_partial"] - rp).sum() <= c["tol"]["loss"]
    # the other outputs do not depend on the loss form
    for k in ("image", "draw", "weights"):
        assert np.array_equal(bits(p1[k]), bits(a[k]))


@pytest.mark.parametrize("S,white", [(S, w) for S in CR.TILE_S for w in (0, 1)])
def test_tile_flags_and_lists(S, white):
    c = CR.case(S, white)
    R, nt = CR.R_CASE, S // 32
    off2, start2 = 100_000, 37
    f = train(S, white, loss0=CR.LOSS0, flags=True, partial=True)                                 # the deterministic mode's outputs
    l = train(S, white, loss0=CR.LOSS0, tiles=True, count2_start=start2, tile_off2=off2)         # the default mode's
    assert np.array_equal(bits(f["draw"]), bits(l["draw"])) and np.array_equal(bits(f["draw"]), bits(default_run(S, white)["draw"]))
    want = CR.dead_tiles(f["draw"], c["raw"])                      # composite.hip's dead rule on the device's own draw and raw
    assert np.array_equal(f["tile_flags"], want)
    live = np.flatnonzero(want).astype(np.int32)
    n = int(l["tile_count"][0])
    print(f"\nS {S} white {white}: {n} of {R * nt} tiles live")
    assert n == len(live) and 0 < n < R * nt
    got = l["tile_list"][:n]
    assert len(set(got.tolist())) == n and np.array_equal(np.sort(got), live)                  # block order only: compared sorted
    assert (l["tile_list"][n:] == -1).all()                                                    # nothing written behind the count
    assert int(l["tile_count2"][0]) == start2 + n
    assert (l["tile_list2"][:start2] == -1).all() and (l["tile_list2"][start2 + n:] == -1).all()
    got2 = l["tile_list2"][start2:start2 + n]
    assert np.array_equal(np.sort(got2), live + off2)           # the same set, shifted (its own counter: its own order of workgroups)
    for lst in (got, got2 - off2):                              # in both lists a workgroup's tiles are ONE ascending run
        wg = lst // (4 * nt)
        starts = np.flatnonzero(np.diff(wg, prepend=-1) != 0)
        assert len(set(wg[starts].tolist())) == len(starts) and (np.diff(lst)[wg[1:] == wg[:-1]] > 0).all()
    per_ray = want.reshape(R, nt)
    assert not per_ray[np.isin(c["cls"], (CR.ALL_ZERO, CR.RGB_OUTSIDE, CR.OWN_PIXEL))].any()   # wholly dead classes
    assert per_ray[np.isin(c["cls"], (CR.UNIFORM, CR.REPEATED_T))].all()
    # behind an opaque front: after six samples with x == 1e-10 exactly the transmittance (1e-10)^6 is zero in float32
    op = np.flatnonzero(c["cls"] == CR.OPAQUE)
    delta, one = np.diff(c["t"][op], axis=1), np.float32(1)
    ex = np.exp(-(c["raw"][op, :-1, 3] * delta).astype(np.float64)).astype(np.float32)
    opaque = (one - (one - ex)) + np.float32(1e-10) == np.float32(1e-10)
    before = np.concatenate([np.zeros((len(op), 1), int), np.cumsum(opaque, axis=1)], axis=1)[:, ::32][:, :nt]     # opaque samples in front of each tile
    behind = before >= 6
    assert not per_ray[op][behind].any()
    if S >= 192:
        assert behind.any() and per_ray[op].any()


@pytest.mark.parametrize("white", [0, 1])
def test_nothing_live_gives_an_empty_list(white):
    from keras_nerf_amd import debug
    rng = np.random.default_rng(5)
    R, S = 13, 96
    raw = rng.random((R, S, 4)).astype(np.float32)
    raw[..., 3] = 0                                                # no density anywhere: w = 0, and sigma == 0 closes the ReLU gate
    t = np.sort(2 + 4 * rng.random((R, S)).astype(np.float32), axis=1)
    out = debug.composite_train(torch.from_numpy(raw).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(rng.random((R, 3)).astype(np.float32)).cuda(),
                                white, 0.1, 0.1, flags=True, tiles=True, count2_start=3, tile_off2=7)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert (out["draw"][..., 3] != 0).all()                        # a gradient there is; it is the tiles that are dead
    assert not out["tile_flags"].any() and int(out["tile_count"][0]) == 0 and int(out["tile_count2"][0]) == 3
    assert (out["tile_list"] == -1).all() and (out["tile_list2"] == -1).all()


def test_entry_rejects_what_the_kernel_cannot_take():
    from keras_nerf_amd import _lib, debug
    z = lambda *s: torch.zeros(s, device="cuda")
    with pytest.raises(_lib.KnerfError):
        debug.composite_train(z(4, 33, 4), z(4, 33), z(4, 3), 0, 1.0, 1.0, flags=True)          # tiles would straddle rays
    with pytest.raises(_lib.KnerfError):
        debug.composite_train(z(1, 1025, 4), z(1, 1025), z(1, 3), 0, 1.0, 1.0)                  # more than 1024 samples per ray


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 8191, 8192, 8193, 24576, 30000])
def test_compact_tiles(n):
    """the exact ascending list, its count and both stats increments against NumPy; nothing written behind the count"""
    from keras_nerf_amd import debug
    rng = np.random.default_rng(n)
    patterns = {"random": rng.choice(np.array([0, 0, 1, 5, -1], np.int32), n), "sparse": (rng.random(n) < 0.01).astype(np.int32),
                "zeros": np.zeros(n, np.int32), "ones": np.ones(n, np.int32)}
    for name, flags in patterns.items():
        dflags = torch.from_numpy(flags).cuda()
        for period, real in ((1, 1), (6, 2), (8, 8), (7, 5)):
            stats = torch.tensor([1000, 5_000_000_000], dtype=torch.int64, device="cuda")
            lst, count = debug.compact_tiles(dflags, period, real, stats)
            lst, count, stats = lst.cpu().numpy(), int(count.cpu()[0]), stats.cpu().numpy()
            want, n_real = CR.compact_reference(flags, period, real)
            assert count == len(want), (name, period, real)
            assert np.array_equal(lst[:count], want) and (lst[count:] == -1).all(), (name, period, real)
            assert stats[0] == 1000 + len(want) and stats[1] == 5_000_000_000 + n_real, (name, period, real, stats)
    lst, count = debug.compact_tiles(torch.from_numpy(patterns["random"]).cuda(), 6, 2, None)      # stats may be null
    assert np.array_equal(lst.cpu().numpy()[:int(count.cpu()[0])], CR.compact_reference(patterns["random"], 6, 2)[0])
