"""Growing a brick baked field, the parts that need no GPU: what the fixture of the GPU tests has, the index plumbing of prune()
(keras_nerf_amd/baked_bricks_grow.py carried_rows, carry_state) on host tensors against tests/baked_bricks_grow_reference.py, where the
names are reached, the argument checks of the Python surface and of the three entry points, and that the arithmetic of resampling and of
the regulariser is one text for both storages (csrc/baked_grow_common.h).  Every condition is stated in tests/README_baked_bricks_grow.md."""
import numpy as np
import pytest

from tests import baked_bricks_grow_reference as W
from tests import baked_bricks_reference as B
from tests import baked_bricks_train_reference as S
from tests import baked_grow_reference as G
from tests import baked_reference as R

RES = (19, 17, 12)                      # the lattice of tests/test_baked_bricks_host.py, rebuilt here with the same seed
LO, HI = (-1.0, -0.8, -0.6), (1.0, 0.8, 0.7)
BRICKS = (4, 8)
DESTINATIONS = ((37, 33, 23), (25, 21, 16), (23, 7, 40), (10, 9, 7), (2, 2, 2))     # 2 R - 1, finer, mixed, coarser, nothing left
THRESHOLDS = (0.0, 10.0)


def lattice(degree, seed=0):
    """random coefficients at EVERY lattice point, sigma > 0 only in two separated blobs: points 6..9 on every axis and points
    (16..17, 14..15, 2..3) next to the +x / +y faces"""
    rng = np.random.default_rng(300 + seed)
    sigma = np.zeros(RES, dtype=np.float32)
    sigma[6:10, 6:10, 6:10] = rng.uniform(5.0, 30.0, (4, 4, 4)).astype(np.float32)
    sigma[16:18, 14:16, 2:4] = rng.uniform(5.0, 30.0, (2, 2, 2)).astype(np.float32)
    K = (degree + 1) ** 2
    co = (rng.standard_normal(RES + (K, 3)) * 0.6).astype(np.float16)
    co[..., 0, :] += np.float16(1.5)
    return sigma, co


def three_blobs(degree):
    """the lattice above and a third blob, the single point (14, 2, 2) with sigma 7: a threshold of 7.5 empties it, and a dilation of
    one cell around it reaches bricks the field does not store (tests/test_baked_bricks_train_host.py)"""
    sigma, co = lattice(degree)
    sigma[14, 2, 2] = np.float32(7.0)
    return sigma, co


def scene(degree, b):
    """(sigma, coefficients, brick_of, n_bricks, brick records) of the two blobs, from the NumPy references"""
    sigma, co = lattice(degree)
    brick_of, n = B.brick_table(R.occupied_cells(sigma), RES, b)
    return sigma, co, brick_of, n, B.bricks_from_dense(G.pack(sigma, co, degree), brick_of, n, RES, b)


def test_the_lattice_is_the_one_of_the_brick_tests():
    from tests.test_baked_bricks_host import RES as theirs, lattice as their_lattice
    assert theirs == RES
    for a, b in zip(lattice(1), their_lattice(1)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("b", BRICKS)
def test_the_fixture_has_what_the_tests_need(b):
    """as a source and on every destination: absent bricks and stored bricks that reach past the lattice"""
    _, _, brick_of, n, bricks = scene(0, b)
    assert (brick_of < 0).any() and B.partial_edge_bricks(brick_of, RES, b).any()
    for res in DESTINATIONS[:3]:
        for thr in THRESHOLDS:
            _, occ, of, n_new, _ = W.resample(bricks, brick_of, RES, b, res, 0, thr)
            assert occ.any() and (of < 0).any() and B.partial_edge_bricks(of, res, b).any(), (res, thr)
            assert n_new == int((of >= 0).sum())
    _, occ, of, _, _ = W.resample(bricks, brick_of, RES, b, (10, 9, 7), 0, 0.0)
    assert occ.any() and B.partial_edge_bricks(of, (10, 9, 7), b).any() and bool((of < 0).any()) == (b == 4)
    sigma, occ, of, n_new, rec = W.resample(bricks, brick_of, RES, b, (2, 2, 2), 0, 0.0)
    assert not occ.any() and n_new == 1 and (of == -1).all() and rec.shape == (1, b ** 3, 16) and not rec.any() and not sigma.any()
    # the threshold matters: it empties cells that are occupied without it
    a = W.resample(bricks, brick_of, RES, b, (25, 21, 16), 0, 0.0)[1]
    c = W.resample(bricks, brick_of, RES, b, (25, 21, 16), 0, 10.0)[1]
    assert c.sum() < a.sum() and not (c & ~a).any()


def _prune_case(degree, b, dilation):
    """the train state of the three blobs, and the one a prune at 7.5 leaves once training has brought the second blob to sigma 0 (the
    second and the third blob are gone, and with them bricks of both sizes), from the references"""
    sigma, co = three_blobs(degree)
    old = W.train_state(sigma, co, b, dilation)
    moved = sigma.copy()
    moved[16:18, 14:16, 2:4] = 0
    cut = W.finished(moved, 7.5)
    assert cut[14, 2, 2] == 0 and cut.any()
    return sigma, co, old, W.train_state(cut, co, b, dilation)


@pytest.mark.parametrize("dilation", [0, 1])
@pytest.mark.parametrize("b", BRICKS)
def test_carried_rows_equal_the_reference(b, dilation):
    import torch
    from keras_nerf_amd.baked_bricks_grow import carried_rows, carry_state
    sigma, co, (_, old_of, n_old, old_flags, old_master), (_, new_of, n_new, new_flags, new_master) = _prune_case(2, b, dilation)
    assert n_new < n_old                                                   # the prune drops a brick
    assert W.train_state(sigma, co, b, 1)[2] > W.train_state(sigma, co, b, 0)[2]           # and dilation adds one
    want_row, want_sigma = W.carried_rows(old_of, old_flags, new_of, new_flags, RES, b)
    got_row, got_sigma = carried_rows(torch.as_tensor(old_of), torch.as_tensor(old_flags), torch.as_tensor(new_of),
                                      torch.as_tensor(new_flags), RES, b)
    assert got_row.dtype == torch.int32 and got_sigma.dtype == torch.bool
    assert np.array_equal(got_row.numpy(), want_row) and np.array_equal(got_sigma.numpy(), want_sigma)
    slot_new = (new_flags & 1) != 0
    assert (want_row >= 0).any() and (want_row[slot_new] >= 0).all()       # (a prune only shrinks the support: every new slot was one)
    assert (want_row[~slot_new] == -1).all() and (want_sigma & ~(want_row >= 0)).sum() == 0
    assert ((want_row >= 0) & ~want_sigma).any() and want_sigma.any()
    # a carried row is the row of the same lattice point
    old_at, new_at = S.row_points(old_of, RES, b), S.row_points(new_of, RES, b)
    kept = want_row >= 0
    assert np.array_equal(old_at[want_row[kept]], new_at[kept])
    # the state moves by these indices: coefficient columns where a row is carried, the sigma column where `sigma` says so
    rng = np.random.default_rng(b + dilation)
    W_ = old_master.shape[1]
    old = rng.standard_normal((old_flags.size, W_)).astype(np.float32)
    start = rng.standard_normal((new_flags.size, W_)).astype(np.float32)
    for with_sigma in (False, True):
        new = torch.as_tensor(start.copy())
        carry_state(got_row, got_sigma if with_sigma else None, torch.as_tensor(old), new)
        want = start.copy()
        want[kept, 1:] = old[want_row[kept], 1:]
        if with_sigma:
            want[want_sigma, 0] = old[want_row[want_sigma], 0]
        assert np.array_equal(new.numpy().view(np.int32), want.view(np.int32))


def test_the_names_are_reached_like_the_brick_optimiser():
    from keras_nerf_amd import baked, baked_bricks_grow, baked_train
    from keras_nerf_amd.baked import BrickBakedField
    from keras_nerf_amd.baked_bricks_train import BrickFieldOptimizer
    for name in ("BrickGridTrainer", "grid_trainer", "resample_bricks", "fit_coarse_to_fine_bricks"):
        assert getattr(baked_train, name) is getattr(baked_bricks_grow, name) is getattr(baked, name), name
    T = baked_bricks_grow.BrickGridTrainer
    assert issubclass(T, BrickFieldOptimizer) and T is not BrickFieldOptimizer
    for name in ("regularize", "tv_weights", "regularized", "prune", "counts", "accumulate", "apply", "train_step", "fit", "finish"):
        assert hasattr(T, name), name
    # and the classes the new surface stays off keep theirs
    for name in ("regularize", "tv_weights", "regularized", "prune"):
        assert not hasattr(BrickFieldOptimizer, name), name
    assert not hasattr(BrickBakedField, "resample") and not hasattr(BrickBakedField, "optimizer")


def _host_field(degree=2, b=8):
    import torch
    from keras_nerf_amd.baked import BrickBakedField
    from keras_nerf_amd.runtime import pack_occupancy
    sigma, _, brick_of, _, bricks = scene(degree, b)
    words = torch.as_tensor(pack_occupancy(R.occupied_cells(sigma)).view(np.int32))
    return BrickBakedField(torch.as_tensor(bricks), torch.as_tensor(brick_of), words, RES, (LO, HI), degree, b, 0.0)


def test_python_surface_refuses_bad_arguments(monkeypatch):
    """every refusal comes before the first launch: the fields here live on the host and every launch is forbidden"""
    import torch
    from keras_nerf_amd import _lib, baked_bricks_grow as M, runtime
    from keras_nerf_amd.baked import BakedField
    from tests.test_baked_quant_host import _host_qfield

    def forbidden(*a, **k):
        raise AssertionError("a refused argument reached a launch")
    monkeypatch.setattr(runtime, "occupancy_words_from_grid", forbidden)
    monkeypatch.setattr(_lib, "load", forbidden)
    field = _host_field()
    dense = BakedField(torch.zeros((27, 16), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), (3, 3, 3), (LO, HI), 0)
    quantized = _host_qfield()[0]
    good = dict(learning_rate_sigma=0.05, learning_rate_sh=0.01)
    for call in (lambda f: M.resample_bricks(f, 9), lambda f: M.grid_trainer(f, **good),
                 lambda f: M.fit_coarse_to_fine_bricks(f, [], 0.0, 1.0, [(None, 1)], **good)):
        with pytest.raises(ValueError, match=r"compact\(\)"):
            call(dense)
        with pytest.raises(ValueError, match=r"dequantize\(\)"):
            call(quantized)
        with pytest.raises(ValueError, match="BrickBakedField"):
            call(None)
    for bad in (1, 1026, (9, 7), (9, 7, 0), 9.0, True):
        with pytest.raises(ValueError, match="resolution"):
            M.resample_bricks(field, bad)
    for bad in (-1.0, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError, match="sigma_threshold"):
            M.resample_bricks(field, 9, sigma_threshold=bad)
    for bad in (2, 16, 8.0, True, 0):
        with pytest.raises(ValueError, match="brick"):
            M.resample_bricks(field, 9, brick=bad)
    for kw in (dict(tv_sigma=-1e-3), dict(tv_sh=float("nan")), dict(tv_epsilon=0.0), dict(tv_epsilon=-1.0), dict(tv_sigma="1")):
        with pytest.raises(ValueError, match="tv_"):
            M.grid_trainer(field, **good, **kw)
    for kw in (dict(learning_rate_sigma=0.0), dict(beta_1=1.0), dict(epsilon=0.0), dict(dilation=9), dict(termination=1.0), dict(step=0.0),
               dict(lanes_per_ray=2)):
        with pytest.raises(ValueError):
            M.grid_trainer(field, **{**good, **kw})
    for bad in (0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="prune_every"):
            M.fit_coarse_to_fine_bricks(field, [], 0.0, 1.0, [(None, 1)], prune_every=bad, **good)
    assert M.check_prune_every(None) is None and M.check_prune_every(np.int64(3)) == 3
    for bad in ([], [(None,)], [(None, -1)], [(None, 1.5)], 5):
        with pytest.raises(ValueError, match="stage"):
            M.fit_coarse_to_fine_bricks(field, [], 0.0, 1.0, bad, **good)
    with pytest.raises(ValueError, match="sigma_threshold"):
        M.fit_coarse_to_fine_bricks(field, [], 0.0, 1.0, [(None, 1)], sigma_threshold=-1.0, **good)
    # with good arguments each gets as far as its first launch
    with pytest.raises(AssertionError, match="reached a launch"):
        M.resample_bricks(field, (10, 9, 7), sigma_threshold=10.0, brick=4)
    with pytest.raises(AssertionError, match="reached a launch"):
        M.grid_trainer(field, tv_sigma=1e-3, **good)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID decided on the host: no device is needed and no pointer is dereferenced"""
    import ctypes as C
    from keras_nerf_amd import _lib
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    p, far = C.c_void_p(4096), C.c_void_p(1 << 40)                       # never dereferenced: every call below is refused first
    nan, inf = float("nan"), float("inf")

    def bricks(res=RES, degree=2, lo=LO, hi=HI, records=p, brick_of=p, bits=p, log2=3, n_bricks=11):
        return _lib.KnerfBakedBricks(records, brick_of, bits, (C.c_int32 * 3)(*res), degree, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), log2,
                                     n_bricks)

    # what knerf_baked_render_bricks refuses of its field
    FIELD = (dict(records=None), dict(brick_of=None), dict(degree=-1), dict(degree=4), dict(res=(1, 17, 12)), dict(res=(19, 1026, 12)),
             dict(res=(19, 17, 0)), dict(hi=(1.0, -0.8, 0.7)), dict(lo=(nan, -0.8, -0.6)), dict(hi=(inf, 0.8, 0.7)), dict(log2=0), dict(log2=1),
             dict(log2=4), dict(log2=-3), dict(n_bricks=0), dict(n_bricks=19), dict(log2=2, n_bricks=76), dict(n_bricks=1 << 40),
             dict(n_bricks=(1 << 64) - 1), dict(res=(1025, 1025, 1025), degree=3, log2=2, n_bricks=(1 << 40) // (64 * 112) + 1))

    def sigma(src, new=(37, 33, 23), thr=0.0, out=far):
        return lib.knerf_baked_resample_bricks_sigma(None, C.byref(src) if src is not None else None,
                                                     (C.c_int32 * 3)(*new) if new is not None else None, thr, out)

    assert sigma(None) == INV
    for bad in FIELD:
        assert sigma(bricks(**bad)) == INV, bad
    for bad in (dict(new=None), dict(new=(1, 33, 23)), dict(new=(37, 33, 1026)), dict(new=(37, 0, 23)), dict(thr=-1.0), dict(thr=nan),
                dict(thr=inf), dict(out=None)):
        assert sigma(bricks(), **bad) == INV, bad

    def records(src, dst, keys=p, thr=0.0, out=far):
        return lib.knerf_baked_resample_bricks(None, C.byref(src) if src is not None else None, C.byref(dst) if dst is not None else None,
                                               keys, thr, out)

    dst = lambda **kw: bricks(**{**dict(res=(37, 33, 23), n_bricks=20, records=None, bits=None), **kw})
    assert records(None, dst()) == INV and records(bricks(), None) == INV
    for bad in FIELD:
        assert records(bricks(**bad), dst()) == INV, bad
        if bad != dict(records=None):                                      # the destination's own record pointer is not read
            change = dict(bad)
            if change.get("n_bricks") in (19, 76):
                change["n_bricks"] = 5 * 5 * 3 + 1 if change.get("log2") != 2 else 10 * 9 * 6 + 1
            assert records(bricks(), dst(**change)) == INV, bad
    for bad in (dict(keys=None), dict(out=None), dict(thr=-1.0), dict(thr=nan), dict(thr=inf)):
        assert records(bricks(), dst(), **bad) == INV, bad
    assert records(bricks(), dst(degree=1)) == INV                          # another degree
    assert records(bricks(), dst(lo=(-1.0, -0.8, -0.5))) == INV and records(bricks(), dst(hi=(1.0, 0.8, 0.75))) == INV       # another box
    # destination records (20 bricks) that overlap the source records (11 bricks), 512 records of 64 bytes each
    at = 1 << 30
    for out in (at, at + 64, at + 11 * 512 * 64 - 1, at - 20 * 512 * 64 + 1):
        assert records(bricks(records=C.c_void_p(at)), dst(), out=C.c_void_p(out)) == INV, out

    def tv(st, keys=p, flags=p, master=p, ws=1e-3, wc=1e-3, eps=1e-6, out=p):
        return lib.knerf_baked_bricks_train_tv(None, C.byref(st) if st is not None else None, keys, flags, master, ws, wc, eps, out)

    state = lambda grad=p, **kw: _lib.KnerfBakedBricksTrain(bricks(**kw), grad)
    assert tv(None) == INV
    for bad in FIELD + (dict(bits=None), dict(grad=None)):
        assert tv(state(**bad)) == INV, bad
    for bad in (dict(keys=None), dict(flags=None), dict(master=None), dict(ws=-1e-3), dict(wc=nan), dict(ws=inf), dict(eps=0.0), dict(eps=nan),
                dict(eps=-1e-6), dict(eps=inf)):
        assert tv(state(), **bad) == INV, bad
    # both weights 0 and nothing to report: KNERF_OK without a launch, for both brick sizes
    assert tv(state(), ws=0.0, wc=0.0, out=None) == 0 and tv(state(log2=2, n_bricks=75), ws=0.0, wc=0.0, out=None) == 0


def test_the_arithmetic_is_one_text_for_both_storages():
    """lerp, the placement, the trilinear step, a record's chunk and the regulariser's column are defined once, in
    csrc/baked_grow_common.h, and both kernel files call them and define none of their own"""
    import os
    import re
    from keras_nerf_amd import baked, build
    csrc = os.path.join(os.path.dirname(os.path.abspath(baked.__file__)), "csrc")
    read = lambda name: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, name)).read())
    header, dense, brick = read("baked_grow_common.h"), read("baked_grow.hip"), read("baked_bricks_grow.hip")
    heads = ("float lerp(", "void place(", "float trilerp(", "uint4 resample_chunk(", "float resample_sigma(", "float tv_term(",
             "float tv_column(", "void tv_store(", "float keep_sigma(")
    for head in heads:
        assert header.count(head) == 1 and head not in dense and head not in brick, head
    for src in (dense, brick):
        assert '#include "baked_grow_common.h"' in src
        for call in ("place(", "resample_chunk(", "tv_column<W>(", "tv_store<W>("):
            assert call in src, call
        assert "__fmul_rn" not in src and "sqrtf" not in src and "half_bits" not in src      # nothing rounds outside the header
    assert "resample_sigma(" in brick
    assert "baked_bricks_grow.hip" in build.SOURCES and "baked_bricks_grow.hip" in build.NO_SPILL and "baked_grow_common.h" in build.HEADERS
