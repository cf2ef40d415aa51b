"""The occupancy grid's host side, no GPU needed: the NumPy mirror of the cell lookup on its edge cases (p exactly at lo and at hi,
NaN, -0, both outside policies), the bit layout knerf_set_occupancy receives, lattice -> cells -> dilation, and argument validation
of the Python API."""
import numpy as np
import pytest

from keras_nerf_amd import runtime
from tests import occupancy_reference as M

LO, HI = (-1.5,) * 3, (1.5,) * 3


def test_scale_is_rounded_once_from_double():
    s = M.scale_of((128, 64, 3), LO, HI)
    assert s.dtype == np.float32
    assert s[0] == np.float32(128 / 3.0) and s[1] == np.float32(64 / 3.0) and s[2] == np.float32(1.0)


def test_points_at_lo_and_at_hi():
    occ = np.ones((128, 128, 128), dtype=bool)
    at_lo = np.array([[-1.5, -1.5, -1.5]], dtype=np.float32)
    at_hi = np.array([[1.5, 1.5, 1.5]], dtype=np.float32)
    # lo: u = 0 exactly, cell 0, inside
    occ0 = np.zeros_like(occ); occ0[0, 0, 0] = True
    assert M.lookup(at_lo, occ0, LO, HI, "empty")[0]
    # hi: u = 3 * fp32(128 / 3) rounds to 128 = c -> outside on every axis
    u = (np.float32(1.5) - np.float32(-1.5)) * M.scale_of((128,) * 3, LO, HI)[0]
    assert np.float32(u) >= 128
    assert not M.lookup(at_hi, occ, LO, HI, "empty")[0]
    assert M.lookup(at_hi, np.zeros_like(occ), LO, HI, "occupied")[0]
    # one axis out is enough
    p = np.array([[0.0, 0.0, 1.5]], dtype=np.float32)
    assert not M.lookup(p, occ, LO, HI, "empty")[0] and M.lookup(p, ~occ, LO, HI, "occupied")[0]


def test_nan_and_negative_zero():
    occ = np.zeros((4, 4, 4), dtype=bool); occ[0, 0, 0] = True
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    nan = np.array([[np.nan, 0.5, 0.5]], dtype=np.float32)
    assert not M.lookup(nan, ~occ, lo, hi, "empty")[0]          # NaN is outside
    assert M.lookup(nan, occ & False, lo, hi, "occupied")[0]
    mz = np.array([[-0.0, -0.0, -0.0]], dtype=np.float32)     # -0 - 0 = -0, u = -0 >= 0: inside, cell 0
    assert M.lookup(mz, occ, lo, hi, "empty")[0]
    assert not M.lookup(np.array([[-1e-7, 0.0, 0.0]], dtype=np.float32), occ, lo, hi, "empty")[0]
    assert not M.lookup(np.array([[np.inf, 0.0, 0.0]], dtype=np.float32), ~occ, lo, hi, "empty")[0]


def test_lookup_picks_the_cell_of_the_bit():
    rng = np.random.default_rng(3)
    occ = rng.random((5, 7, 9)) < 0.5
    lo, hi = (-1.0, -2.0, 0.5), (1.0, 3.0, 2.0)
    p = rng.uniform(-3, 4, (20000, 3)).astype(np.float32)
    live = M.lookup(p, occ, lo, hi, "empty")
    s = M.scale_of(occ.shape, lo, hi)
    u = ((p - np.float32(lo)) * s).astype(np.float32)
    for q in range(0, 20000, 97):
        if np.all((u[q] >= 0) & (u[q] < occ.shape)):
            i, j, k = (int(np.floor(x)) for x in u[q])
            assert live[q] == occ[i, j, k]
        else:
            assert not live[q]


def test_bit_layout():
    occ = np.zeros((3, 5, 7), dtype=bool)
    occ[0, 0, 0] = occ[0, 0, 31 - 28 + 28 - 7 * 4] = True     # b = 3
    occ[1, 0, 4] = True                                        # b = 35 + 4 = 39 -> word 1, bit 7
    occ[2, 4, 6] = True                                        # b = 104 = the last cell -> word 3, bit 8
    w = M.pack(occ)
    assert w.dtype == np.uint32 and len(w) == 4
    assert w[0] == (1 | 1 << 3) and w[1] == 1 << 7 and w[2] == 0 and w[3] == 1 << 8
    rng = np.random.default_rng(0)
    for shape in ((1, 1, 1), (3, 5, 7), (16, 16, 16), (2, 3, 33)):
        g = rng.random(shape) < 0.4
        assert np.array_equal(runtime.pack_occupancy(g), M.pack(g))
        assert np.array_equal(runtime.unpack_occupancy(M.pack(g), shape), g)


def test_lattice_cells_and_dilation():
    sig = np.zeros((9, 9, 9), dtype=np.float32)
    sig[4, 4, 4] = 2.0                     # one lattice point: the 8 cells around it
    c = M.corner_cells(sig, 0.0)
    assert c.shape == (8, 8, 8) and c.sum() == 8 and c[3:5, 3:5, 3:5].all()
    assert M.corner_cells(sig, 2.0).sum() == 0          # strictly greater
    d1 = M.dilate(c, 1)
    assert d1.sum() == 64 and d1[2:6, 2:6, 2:6].all()
    assert M.dilate(c, 8).all()
    sig[0, 0, 0] = 1.0
    g = M.grid_from_lattice(sig, 0.5, 2)
    assert g[0, 0, 0] and g[2, 2, 2] and not g[3, 0, 0] and g[1:7, 1:7, 1:7].all()
    # dilation == OR over the lattice box [i - d, i + 1 + d] (what occ_build_kernel reads)
    rng = np.random.default_rng(1)
    sig = (rng.random((6, 7, 8)) > 0.97).astype(np.float32)
    for d in (0, 1, 3):
        g = M.grid_from_lattice(sig, 0.0, d)
        for i, j, k in [(0, 0, 0), (2, 3, 4), (4, 5, 6), (1, 0, 6)]:
            box = sig[max(0, i - d):i + 2 + d, max(0, j - d):j + 2 + d, max(0, k - d):k + 2 + d]
            assert g[i, j, k] == bool((box > 0).any())


def test_occupancy_spec_validation():
    ok = np.ones((4, 4, 4), dtype=bool)
    words, cells, lo, hi, oe = runtime.occupancy_spec(ok, LO, HI, "empty")
    assert cells == (4, 4, 4) and oe == 1 and len(words) == 2 and words.dtype == np.uint32
    for bad in (np.ones((4, 4), dtype=bool), np.ones((4, 4, 4), dtype=np.float32), np.ones((1025, 1, 1), dtype=bool),
                np.ones((0, 4, 4), dtype=bool)):
        with pytest.raises(ValueError):
            runtime.occupancy_spec(bad, LO, HI)
    for lo, hi in (((1, 1, 1), (1, 2, 2)), ((0, 0), (1, 1)), ((0, 0, np.nan), (1, 1, 1)), ((0, 0, 0), (1, 1, np.inf)), (3, 4)):
        with pytest.raises(ValueError):
            runtime.occupancy_spec(ok, lo, hi)
    with pytest.raises(ValueError):
        runtime.occupancy_spec(ok, LO, HI, "maybe")


def test_occupancy_from_grid_validation():
    import torch
    with pytest.raises(ValueError):
        runtime.occupancy_from_grid(np.zeros((4, 4, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        runtime.occupancy_from_grid(torch.zeros((4, 4, 4)))          # a host tensor


def test_nerf_argument_validation_without_a_gpu():
    from keras_nerf_amd.model.nerf.nerf import NeRF
    n = NeRF()
    for kw in (dict(resolution=0), dict(resolution=1025), dict(resolution=(8, 8)), dict(resolution=2.5), dict(dilation=9),
               dict(dilation=-1), dict(dilation=1.5), dict(outside="none"), dict(bounds=((1,) * 3, (0,) * 3)),
               dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            n.build_occupancy_grid(**kw)
    with pytest.raises(ValueError):
        n.set_occupancy_grid("fine", np.ones((2, 2), dtype=bool))
    with pytest.raises(ValueError):
        n.set_occupancy_grid("fine", np.ones((2, 2, 2), dtype=bool), bounds=((0, 0, 0), (1, 1, 0)))
    with pytest.raises(ValueError):
        n.set_occupancy_grid("fine", np.ones((2, 2, 2), dtype=bool), outside="inside")
    with pytest.raises(RuntimeError):                  # valid arguments, but not compiled
        n.build_occupancy_grid()
