"""Point queries of baked fields, the parts that need no GPU (keras_nerf_amd/baked_query.py, csrc/baked_query.hip's host side,
tests/baked_query_reference.py): the reference against itself, the wiring, and every refusal.  tests/README_baked_query.md"""
import ctypes as C
import os

import numpy as np
import pytest

import baked_query_reference as R
from keras_nerf_amd import _lib, baked_query
from keras_nerf_amd.baked import n_coefficients, pack_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_field(res, degree, seed=0):
    rng = np.random.default_rng(seed)
    sigma = rng.uniform(0.0, 4.0, res).astype(np.float32)
    co = rng.normal(0.0, 0.6, res + (n_coefficients(degree), 3)).astype(np.float16)
    return sigma, co


def test_reference_gradient_agrees_with_central_differences_inside_cells():
    res, lo, hi = (5, 6, 7), (-1.0, -0.5, 0.25), (1.5, 0.75, 2.0)
    sigma, co = random_field(res, 1)
    rng = np.random.default_rng(1)
    cell = np.stack([rng.integers(0, r - 1, 200) for r in res], axis=1)
    fr = rng.uniform(0.2, 0.8, (200, 3))
    size = (np.asarray(hi) - np.asarray(lo)) / (np.asarray(res) - 1)
    p = (np.asarray(lo) + (cell + fr) * size).astype(np.float32)
    out = R.query(sigma, co, lo, hi, p)
    assert out["inside"].all()
    h = 2.0 ** -7                                                    # exact in float32 beside coordinates of this size: |p| < 2, ulp 2^-23
    for ax in range(3):
        e = np.zeros(3, dtype=np.float32)
        e[ax] = h
        up, dn = R.query(sigma, co, lo, hi, p + e), R.query(sigma, co, lo, hi, p - e)
        moved = (p + e)[:, ax].astype(np.float64) - (p - e)[:, ax].astype(np.float64)
        fd = (up["sigma"] - dn["sigma"]) / moved
        # sigma is linear along an axis inside a cell, so the difference quotient IS the derivative up to the float32 lookup's
        # rounding of u (2 roundings of relative size 2^-24 on a value below 8, seen through a slope below 4 scale / h apart)
        assert np.abs(fd - out["grad"][:, ax]).max() < 1e-3
        assert np.abs(out["grad"][:, ax]).max() > 0.1


def test_reference_returns_the_stored_values_at_lattice_points():
    """box [-1, 1]^3 with R = 5: cell 0.5, scale 2, every step exact"""
    res, lo, hi = (5, 5, 5), (-1.0,) * 3, (1.0,) * 3
    sigma, co = random_field(res, 2)
    assert np.array_equal(R.lattice_scale(res, lo, hi), np.full(3, 2.0, dtype=np.float32))
    idx = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    p = (idx * 0.5 - 1.0).astype(np.float32)
    out = R.query(sigma, co, lo, hi, p)
    assert out["inside"].all()
    assert np.array_equal(out["sigma"], sigma.reshape(-1).astype(np.float64))
    y0 = 0.5 / np.sqrt(np.pi)
    assert np.array_equal(out["rgb"], np.clip(co.reshape(-1, 9, 3)[:, 0].astype(np.float64) * y0, 0.0, 1.0))
    assert np.array_equal(R.grid_points(res, lo, hi), p)
    # outside on each side, and a NaN coordinate: exact zeros
    bad = np.array([[-1.5, 0, 0], [0, 1.25, 0], [0, 0, -1.000001], [1.000001, 0, 0], [np.nan, 0, 0]], dtype=np.float32)
    out = R.query(sigma, co, lo, hi, bad, np.array([0.0, 0.0, 1.0]))
    assert not out["inside"].any()
    assert all(not out[k].any() for k in ("sigma", "rgb", "grad", "sigma_abs", "rgb_abs", "grad_abs"))


def test_reference_direction_rules():
    res, lo, hi = (5, 5, 5), (-1.0,) * 3, (1.0,) * 3
    sigma, co = random_field(res, 3)
    p = np.array([[0.1, -0.3, 0.2]] * 4, dtype=np.float32)
    none = R.query(sigma, co, lo, hi, p)
    d = np.array([[0.0, 0.0, 0.0], [np.nan, 1.0, 0.0], [3e38, 3e38, 0.0], [0.0, 0.0, 2.0]], dtype=np.float32)
    per = R.query(sigma, co, lo, hi, p, d)
    assert np.array_equal(per["rgb"][:3], none["rgb"][:3])          # length 0, NaN, overflowing: the DC term alone
    unit = R.query(sigma, co, lo, hi, p, np.array([0.0, 0.0, 1.0], dtype=np.float32))
    assert np.array_equal(per["rgb"][3], unit["rgb"][3]) and not np.array_equal(unit["rgb"][3], none["rgb"][3])


def test_symbols_sources_and_header():
    from keras_nerf_amd import build
    hdr = open(os.path.join(ROOT, "include", "knerf.h")).read()
    for name in ("knerf_baked_query", "knerf_baked_query_bricks", "knerf_baked_query_qbricks"):
        assert name in _lib.SIGNATURES and f"int {name}(" in hdr
        assert hasattr(_lib.load(), name)
    assert "typedef struct knerf_baked_query_spec" in hdr
    assert "baked_query.hip" in build.SOURCES and "baked_query.hip" in build.NO_SPILL and "baked_query.hip" not in build.SLICED
    # the ctypes struct is the header's struct, field for field
    body = hdr.split("typedef struct knerf_baked_query_spec {", 1)[1].split("} knerf_baked_query_spec;", 1)[0]
    import re
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.KnerfBakedQuerySpec._fields_]
    from keras_nerf_amd.baked import BakedField, BrickBakedField
    from keras_nerf_amd.baked_quant import QuantizedBrickField
    for cls in (BakedField, BrickBakedField, QuantizedBrickField):
        for m in ("query", "density_grid", "extract_mesh"):
            assert callable(getattr(cls, m))


def host_fields(degree=2):
    """the three storages over CPU tensors: enough for everything that is decided before the device is touched"""
    import torch
    from keras_nerf_amd import baked
    from keras_nerf_amd.baked_quant import QuantizedBrickField, quantized_record_bytes
    from keras_nerf_amd.runtime import pack_occupancy
    res, bounds = (5, 6, 7), ((-1.0, -0.5, 0.25), (1.5, 0.75, 2.0))
    sigma, co = random_field(res, degree)
    occ = np.ones(tuple(r - 1 for r in res), dtype=bool)
    words = torch.as_tensor(pack_occupancy(occ).view(np.int32))
    rec = pack_records(sigma, co)
    dense = baked.BakedField(torch.as_tensor(rec), words, res, bounds, degree)
    brick_of, n = baked.brick_table(occ, res, 4)
    bricks = baked.bricks_from_dense(rec, brick_of, n, res, 4)
    brick = baked.BrickBakedField(torch.as_tensor(bricks), torch.as_tensor(brick_of), words, res, bounds, degree, 4)
    q = QuantizedBrickField(torch.zeros((n, 64, quantized_record_bytes(degree)), dtype=torch.uint8), torch.zeros((n,), dtype=torch.int32),
                            brick._brick_of, words, res, bounds, degree, 4)
    return dense, brick, q


def test_every_value_error_is_raised_before_the_device():
    pts = np.zeros((4, 3), dtype=np.float32)
    for f in host_fields(2):
        quant = type(f).__name__ == "QuantizedBrickField"
        for bad in (dict(points=np.zeros((4, 2))), dict(points=np.zeros(())), dict(points=np.zeros((4,))), dict(points="abc"),
                    dict(directions=np.zeros((4, 2))), dict(directions=np.zeros((5, 3))), dict(directions=np.zeros((2, 4, 3))),
                    dict(directions=np.zeros(())), dict(lanes_per_point=3), dict(lanes_per_point=2 if not quant else 4),
                    dict(lanes_per_point=True), dict(lanes_per_point=1.0), dict(lanes_per_point=-1)):
            kw = dict(points=pts)
            kw.update(bad)
            with pytest.raises(ValueError):
                f.query(**kw)
        for bad in (dict(resolution=1), dict(resolution=(4, 4)), dict(resolution=(4, 4, 1)), dict(resolution=4.0), dict(resolution=True),
                    dict(resolution=(2048, 2048, 1024)), dict(bounds=((0, 0, 0), (1, 1, 0))), dict(bounds=((0, 0, 0), (1, 1))),
                    dict(bounds=((0, 0, 0), (1, 1, np.inf))), dict(bounds=((np.nan, 0, 0), (1, 1, 1))), dict(bounds=(0, 1)),
                    dict(bounds=((-3e38,) * 3, (3e38,) * 3)), dict(direction=np.zeros((2, 3))), dict(direction=np.zeros(4))):
            with pytest.raises(ValueError):
                f.density_grid(**bad)
            if "direction" not in bad:
                with pytest.raises(ValueError):
                    f.extract_mesh(0.5, **bad)
        for thr in (None, "1", np.nan, np.inf, True):
            with pytest.raises(ValueError):
                f.extract_mesh(thr)
    with pytest.raises(ValueError):
        baked_query.query(object(), pts)
    # degree 1: the dense and brick storages have a pair, the quantised one has no group
    d1, b1, q1 = host_fields(1)
    assert baked_query.check_lanes(d1, 2) == 2 and baked_query.check_lanes(b1, 0) == 0
    with pytest.raises(ValueError):
        baked_query.check_lanes(q1, 2)
    # what the checks hand on
    assert baked_query.check_query_args(d1, np.zeros((2, 5, 3)), np.zeros((5, 3)))[:3] == ((2, 5), 10, 3)
    assert baked_query.check_query_args(d1, np.zeros(3), np.zeros((1, 3)))[:3] == ((), 1, 1)
    assert baked_query.check_query_args(d1, np.zeros((0, 3)))[:3] == ((0,), 0, 0)
    assert baked_query.check_grid_args(d1) == (d1.resolution, d1.bounds[0], d1.bounds[1], True)
    assert baked_query.check_grid_args(d1, 9) == ((9, 9, 9), d1.bounds[0], d1.bounds[1], False)
    assert baked_query.check_grid_args(d1, None, ((0, 0, 0), (1, 1, 1)))[3] is False


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID decided on the host: no device is needed and no pointer is dereferenced"""
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    p, p2 = C.c_void_p(1 << 20), C.c_void_p(1 << 30)
    LO, HI = (-1.0, -0.5, 0.25), (1.5, 0.75, 2.0)
    f3 = lambda v: None if v is None else (C.c_float * 3)(*v)
    lanes = lambda n: n << _lib.BAKED_LANES_SHIFT
    nan, inf = float("nan"), float("inf")

    def spec(points=p, n=0, gres=None, glo=None, ghi=None, directions=None, per_point=0, flags=0, sigma=p, rgb=None, gradient=None, **_):
        return _lib.KnerfBakedQuerySpec(points, n, None if gres is None else (C.c_int32 * 3)(*gres), f3(glo), f3(ghi), directions, per_point,
                                        flags, sigma, rgb, gradient)

    def dense(null=False, nospec=False, res=(19, 17, 12), degree=2, lo=LO, hi=HI, records=p, **kw):
        f = _lib.KnerfBakedField(records, None, (C.c_int32 * 3)(*res), degree, f3(lo), f3(hi))
        s = spec(**kw)
        return lib.knerf_baked_query(None, None if null else C.byref(f), None if nospec else C.byref(s))

    def bricks(res=(19, 17, 12), degree=2, lo=LO, hi=HI, records=p, brick_of=p, log2=3, n_bricks=11, **_):
        return _lib.KnerfBakedBricks(records, brick_of, None, (C.c_int32 * 3)(*res), degree, f3(lo), f3(hi), log2, n_bricks)

    def brick(null=False, nospec=False, **kw):
        f, s = bricks(**kw), spec(**kw)
        return lib.knerf_baked_query_bricks(None, None if null else C.byref(f), None if nospec else C.byref(s))

    def quant(null=False, nospec=False, exponents=p2, **kw):
        f, s = _lib.KnerfBakedQBricks(bricks(**kw), exponents), spec(**kw)
        return lib.knerf_baked_query_qbricks(None, None if null else C.byref(f), None if nospec else C.byref(s))

    # good arguments and no point: KNERF_OK without a launch
    for call in (dense, brick, quant):
        assert call() == 0 and call(rgb=p, gradient=p, sigma=None) == 0 and call(directions=p, per_point=1, rgb=p) == 0
        assert call(flags=lanes(1)) == 0 and call(degree=3, flags=lanes(4)) == 0 and call(degree=0) == 0
    assert dense(flags=lanes(4)) == 0 and brick(degree=1, flags=lanes(2)) == 0 and quant(flags=lanes(2)) == 0
    assert brick(log2=2, n_bricks=75) == 0
    # (a well-formed grid always has points, so it launches: only its refusals can be shown here)
    grid = dict(points=None, gres=(4, 5, 6), glo=(0, 0, 0), ghi=(1, 1, 1))
    field_errors = (dict(null=True), dict(records=None), dict(degree=-1), dict(degree=4), dict(res=(1, 17, 12)), dict(res=(19, 1026, 12)),
                    dict(hi=(1.0, -0.8, 3.0)), dict(lo=(nan, -0.5, 0.25)), dict(hi=(inf, 0.75, 2.0)))
    brick_errors = (dict(brick_of=None), dict(log2=1), dict(log2=4), dict(n_bricks=0), dict(n_bricks=19))
    query_errors = (
        dict(nospec=True), dict(sigma=None), dict(points=None), dict(grid, points=p),
        dict(grid, gres=None), dict(grid, glo=None), dict(grid, ghi=None), dict(grid, gres=(1, 5, 6)), dict(grid, gres=(4, 5, 0)),
        dict(grid, gres=(2048, 2048, 513)), dict(grid, gres=(1 << 30, 1 << 30, 1 << 30)), dict(grid, ghi=(1, 1, inf)),
        dict(grid, glo=(nan, 0, 0)), dict(grid, ghi=(1, 0, 1)), dict(grid, ghi=(1, -1, 1)), dict(grid, glo=(-3e38,) * 3, ghi=(3e38,) * 3),
        dict(flags=1), dict(flags=2), dict(flags=1 << 12), dict(flags=lanes(3)), dict(flags=lanes(8)), dict(degree=0, flags=lanes(2)),
        dict(degree=3, flags=lanes(2)), dict(per_point=2), dict(per_point=-1), dict(n=1 << 36), dict(n=(1 << 64) - 1))
    for call, more in ((dense, (dict(flags=lanes(2)), dict(degree=1, flags=lanes(4)))),
                       (brick, brick_errors + (dict(flags=lanes(2)), dict(degree=1, flags=lanes(4)))),
                       (quant, brick_errors + (dict(exponents=None), dict(flags=lanes(4)), dict(degree=1, flags=lanes(2))))):
        for bad in field_errors + query_errors + more:
            assert call(**bad) == INV, (call.__name__, bad)
