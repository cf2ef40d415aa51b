"""The 8-bit codec of brick baked fields, the parts that need no GPU: the package's NumPy mirrors (keras_nerf_amd/baked_quant.py
quantize_bricks, dequantize_bricks) against tests/baked_quant_reference.py, the properties of the format (fp16-exact decoding, the error
bound, untouched sigma, zero padding, idempotence), special values, the host-side reader of format-3 files, and every refusal of the
Python surface and of the three entry points.  Every condition is stated in tests/README_baked_quant.md."""
import numpy as np
import pytest

from tests import baked_bricks_reference as B
from tests import baked_quant_reference as Q
from tests import baked_reference as R
from tests.test_baked_bricks_host import BRICKS, HI, LO, RES, lattice

_scenes = {}


def qscene(degree, b):
    """(sigma, scaled coefficients, occupied cells, brick_of, n_bricks, brick records) of the quantisation test lattice, from the NumPy
    references; computed once per case and never changed"""
    if (degree, b) not in _scenes:
        from tests import baked_grow_reference as G
        sigma, co = Q.scaled_lattice(*lattice(degree), b)
        occ = R.occupied_cells(sigma)
        brick_of, n = B.brick_table(occ, RES, b)
        bricks = B.bricks_from_dense(G.pack(sigma, co, degree), brick_of, n, RES, b)
        _scenes[(degree, b)] = (sigma, co, occ, brick_of, n, bricks)
    return _scenes[(degree, b)]


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_package_mirrors_equal_the_reference_and_the_format_holds(degree, b):
    from keras_nerf_amd import baked, baked_quant
    bricks = qscene(degree, b)[5]
    K = (degree + 1) ** 2
    want_q, want_e = Q.quantize(bricks, degree)
    got_q, got_e = baked.quantize_bricks(bricks, degree)
    assert baked.quantized_record_bytes(degree) == Q.QRECORD_BYTES[degree] == want_q.shape[2] == (8, 16, 32, 64)[degree]
    assert got_q.dtype == np.uint8 and got_e.dtype == np.uint32 and got_q.shape == want_q.shape and got_e.shape == (bricks.shape[0],)
    assert np.array_equal(got_q, want_q) and np.array_equal(got_e, want_e)
    want_d = Q.dequantize(want_q, want_e, degree)
    got_d = baked.dequantize_bricks(got_q, got_e, degree)
    assert got_d.dtype == np.uint8 and got_d.shape == bricks.shape and np.array_equal(got_d, want_d)
    # sigma untouched; padding and unused exponent bytes zero
    assert np.array_equal(got_q[:, :, :4], bricks[:, :, :4]) and np.array_equal(got_d[:, :, :4], bricks[:, :, :4])
    assert not got_q[:, :, 4 + 3 * K:].any() and not got_d[:, :, 4 + 6 * K:].any()
    assert not (got_e >> np.uint32(8 * (degree + 1))).any() if degree < 3 else True
    # every decoded value is exactly an fp16 number (Q.dequantize asserts it as well) and |c - dec| <= 2^(e-1) everywhere
    dec = Q.decoded(got_q, got_e, degree)
    assert np.array_equal(dec.astype(np.float16).astype(np.float64), dec)
    assert np.array_equal(Q.coefficients(got_d, degree), dec)
    e = Q.exponents_of(got_e, degree)
    assert e.min() >= -24 and e.max() <= 9
    half_step = np.stack([2.0 ** (e[:, Q.band(k)] - 1.0) for k in range(K)], axis=-1)[:, None, :, None]
    c = Q.coefficients(bricks, degree)
    assert (np.abs(c - dec) <= half_step).all()
    M = np.stack([np.abs(c[:, :, [k for k in range(K) if Q.band(k) == l]]).reshape(len(c), -1).max(axis=1) for l in range(degree + 1)], axis=-1)
    big = e > -24
    assert (2.0 ** (e - 1.0) < M / 127.0)[big].all() and big.any()
    # the codec does something, and is idempotent
    assert (dec != c)[c != 0].mean() > 0.9 and np.abs(dec).max() > 0
    again_q, again_e = baked.quantize_bricks(got_d, degree)
    assert np.array_equal(again_q, got_q) and np.array_equal(again_e, got_e)
    assert baked_quant.QLANES[degree][0] == 1


def _special_bricks(degree=2):
    """one brick of 64 places per special value: (records, {name: brick})"""
    K = (degree + 1) ** 2
    names = ["nan", "inf", "-inf", "65504", "subnormal", "-0", "zero band", "exact", "next"]
    co = np.zeros((len(names), 64, K, 3), dtype=np.float16)
    rng = np.random.default_rng(5)
    co[:] = (rng.standard_normal(co.shape) * 0.25).astype(np.float16)
    at = {n: i for i, n in enumerate(names)}
    co[at["nan"], 3, 0, 1] = np.nan
    co[at["inf"], 5, 1, 0] = np.inf
    co[at["-inf"], 5, 2, 2] = -np.inf
    co[at["65504"], 9, 4, 0] = 65504.0
    co[at["65504"], 10, 4, 1] = -65504.0
    co[at["subnormal"]] = (rng.integers(-40, 41, co[0].shape) * 2.0 ** -24).astype(np.float16)            # |c| <= 40 x 2^-24
    co[at["-0"], :, 0, :] = np.float16(-0.0)
    co[at["-0"], 7, 0, 0] = np.float16(0.5)
    co[at["zero band"], :, 1:4, :] = 0
    co[at["exact"], :, 1:4, :] *= np.float16(0.1)
    co[at["exact"], 11, 2, 1] = np.float16(127.0 * 2.0 ** -3)                                            # M = 127 x 2^-3 exactly
    co[at["next"], :, 1:4, :] *= np.float16(0.1)
    co[at["next"], 11, 2, 1] = np.nextafter(np.float16(127.0 * 2.0 ** -3), np.float16(np.inf))
    rec = np.zeros((len(names), 64, Q.RECORD_BYTES[degree]), dtype=np.uint8)
    rec[:, :, :4] = rng.uniform(0, 9, (len(names), 64)).astype(np.float32).view(np.uint8).reshape(len(names), 64, 4)
    rec[:, :, 4:4 + 6 * K] = co.reshape(len(names), 64, 3 * K).view(np.uint8)
    return rec, at, co


def test_special_values():
    from keras_nerf_amd import baked
    rec, at, co = _special_bricks()
    q, e = baked.quantize_bricks(rec, 2)
    want_q, want_e = Q.quantize(rec, 2)
    assert np.array_equal(q, want_q) and np.array_equal(e, want_e)
    ex = Q.exponents_of(e, 2)
    qi = q[:, :, 4:31].view(np.int8).reshape(len(rec), 64, 9, 3)
    dec = Q.decoded(q, e, 2)
    assert np.isfinite(dec).all()
    assert qi[at["nan"], 3, 0, 1] == 0 and ex[at["nan"], 0] < 9                      # a NaN is 0 and does not enter the maximum
    assert qi[at["inf"], 5, 1, 0] == 127 and ex[at["inf"], 1] == 9 and qi[at["-inf"], 5, 2, 2] == -127 and ex[at["-inf"], 1] == 9
    assert qi[at["65504"], 9, 4, 0] == 127 and qi[at["65504"], 10, 4, 1] == -127 and ex[at["65504"], 2] == 9
    assert dec[at["65504"], 9, 4, 0] == 65024.0
    # fp16 subnormals: e = -24 and the codec is the identity
    assert (ex[at["subnormal"]] == -24).all() and np.array_equal(dec[at["subnormal"]], co[at["subnormal"]].astype(np.float64))
    assert np.abs(qi[at["subnormal"]]).max() > 1
    zeros = qi[at["-0"], :, 0, :].copy()
    zeros[7, 0] = 0
    assert not zeros.any() and not np.signbit(dec[at["-0"], :, 0, :]).any() and qi[at["-0"], 7, 0, 0] != 0
    assert ex[at["zero band"], 1] == -24 and not qi[at["zero band"], :, 1:4, :].any()
    assert ex[at["exact"], 1] == -3 and qi[at["exact"], 11, 2, 1] == 127 and ex[at["next"], 1] == -2 and qi[at["next"], 11, 2, 1] == 64
    # the properties hold here too
    d = baked.dequantize_bricks(q, e, 2)
    assert np.array_equal(d, Q.dequantize(q, e, 2))
    q2, e2 = baked.quantize_bricks(d, 2)
    assert np.array_equal(q2, q) and np.array_equal(e2, e)


def _host_field(degree=2, b=4, thr=0.5):
    import torch
    from keras_nerf_amd.baked import BrickBakedField
    from keras_nerf_amd.runtime import pack_occupancy
    sigma, co, occ, brick_of, n, bricks = qscene(degree, b)
    words = pack_occupancy(occ).view(np.int32)
    field = BrickBakedField(torch.as_tensor(bricks), torch.as_tensor(brick_of), torch.as_tensor(words), RES, (LO, HI), degree, b, thr)
    return field, bricks, brick_of, words


def _host_qfield(degree=2, b=4, thr=0.5):
    import torch
    from keras_nerf_amd.baked_quant import QuantizedBrickField
    field, bricks, brick_of, words = _host_field(degree, b, thr)
    q, e = Q.quantize(bricks, degree)
    qf = QuantizedBrickField(torch.as_tensor(q), torch.as_tensor(e.view(np.int32)), field._brick_of, field._words, RES, (LO, HI), degree, b, thr)
    return qf, q, e, brick_of, words


def test_save_writes_what_the_reader_reads(tmp_path):
    import torch
    from keras_nerf_amd import baked
    from keras_nerf_amd.baked import BakedField, BrickBakedField, QuantizedBrickField
    qf, q, e, brick_of, words = _host_qfield()
    n = q.shape[0]
    assert qf.brick == 4 and qf.n_bricks == n and qf.resolution == RES and qf.bounds == (LO, HI) and qf.sh_degree == 2
    assert qf.sigma_threshold == 0.5 and qf.nbytes == q.nbytes + e.nbytes + brick_of.nbytes + words.nbytes
    assert qf.exponents.dtype == torch.int32 and np.array_equal(qf.exponents.numpy().view(np.uint32), e)
    assert tuple(qf.brick_of.shape) == brick_of.shape and np.array_equal(qf.occupied.numpy(), qscene(2, 4)[2])
    assert len(qf.cell_size) == 3 and qf.device.type == "cpu"
    path = str(tmp_path / "scene")
    qf.save(path)
    got = baked.read_quantized_brick_file(path)
    assert got["records"].dtype == np.uint8 and np.array_equal(got["records"], q)
    assert got["exponents"].dtype == np.uint32 and np.array_equal(got["exponents"], e)
    assert np.array_equal(got["brick_of"], brick_of) and np.array_equal(got["words"], words)
    assert got["brick"] == 4 and got["sigma_threshold"] == 0.5 and got["resolution"] == RES and got["n_bricks"] == n and got["sh_degree"] == 2
    with np.load(path) as z:
        assert int(z["format"]) == 3 and int(z["quant_bits"]) == 8 and z["records"].shape == (n, 64, 32)
    again = baked.load_field(path, device="cpu")
    assert isinstance(again, QuantizedBrickField) and torch.equal(again._records, qf._records) and torch.equal(again.exponents, qf.exponents)
    assert torch.equal(QuantizedBrickField.load(path, device="cpu")._records, qf._records)
    # the readers of the other formats keep refusing format 3
    with pytest.raises(ValueError, match="format"):
        baked.read_brick_file(path)
    with pytest.raises(ValueError, match="format"):
        BrickBakedField.load(path, device="cpu")
    with pytest.raises(ValueError, match="format"):
        BakedField.load(path, device="cpu")
    # and the format-3 reader refuses a format-2 file
    two = str(tmp_path / "two")
    _host_field()[0].save(two)
    with pytest.raises(ValueError, match="format"):
        baked.read_quantized_brick_file(two)


def _file(path, b=8, degree=1, **change):
    """a format-3 file written with NumPy from the references; `change` replaces or (value None) drops keys"""
    from keras_nerf_amd.runtime import pack_occupancy
    sigma, co, occ, brick_of, n, bricks = qscene(degree, b)
    q, e = Q.quantize(bricks, degree)
    data = dict(format=np.int32(3), records=q, exponents=e, quant_bits=np.int32(8), brick_of=brick_of,
                words=pack_occupancy(occ).view(np.int32), brick=np.int32(b), resolution=np.asarray(RES, dtype=np.int32),
                lo=np.asarray(LO, dtype=np.float64), hi=np.asarray(HI, dtype=np.float64), sh_degree=np.int32(degree),
                sigma_threshold=np.float64(0.0))
    for k, v in change.items():
        if v is None:
            del data[k]
        else:
            data[k] = v(data[k]) if callable(v) else v
    with open(path, "wb") as f:
        np.savez(f, **data)
    return data


def _exp_byte(brick, l, value):
    def f(e):
        e = e.copy()
        e[brick] = (int(e[brick]) & ~(0xFF << (8 * l))) | ((value & 0xFF) << (8 * l))
        return e
    return f


def _set(i, value):
    def f(t):
        t = t.copy(); flat = t.reshape(-1)
        flat[np.nonzero(flat >= 0)[0][i]] = value
        return t
    return f


def test_reader_refuses_damaged_files(tmp_path, monkeypatch):
    """each kind of damage is a ValueError from the host-side reader; QuantizedBrickField.load and load_field go through the same reader
    before they touch a device (torch.as_tensor is never reached: the test forbids it)"""
    import torch
    from keras_nerf_amd import baked
    from keras_nerf_amd.baked import QuantizedBrickField
    good = str(tmp_path / "good.npz")
    data = _file(good)
    got = baked.read_quantized_brick_file(good)
    assert np.array_equal(got["records"], data["records"]) and np.array_equal(got["exponents"], data["exponents"])
    n = data["records"].shape[0]
    damage = {
        "no exponents": dict(exponents=None), "no quant_bits": dict(quant_bits=None), "no records": dict(records=None),
        "no brick table": dict(brick_of=None), "no bits": dict(words=None), "no format": dict(format=None),
        "quant_bits 4": dict(quant_bits=np.int32(4)), "float quant_bits": dict(quant_bits=np.float64(8.0)),
        "format 2": dict(format=np.int32(2)), "format 4": dict(format=np.int32(4)),
        "exponent byte 10": dict(exponents=_exp_byte(2, 1, 10)), "exponent byte -25": dict(exponents=_exp_byte(0, 0, -25)),
        "exponents a brick short": dict(exponents=lambda e: e[:-1]), "exponents a brick more": dict(exponents=lambda e: np.concatenate([e, e[:1]])),
        "int32 exponents": dict(exponents=lambda e: e.view(np.int32)), "int64 exponents": dict(exponents=lambda e: e.astype(np.int64)),
        "exponents [n, 1]": dict(exponents=lambda e: e.reshape(-1, 1)),
        "records in the unquantised size": dict(records=lambda r: np.zeros(r.shape[:2] + (32,), dtype=np.uint8)),
        "float records": dict(records=lambda r: r.astype(np.float32)), "a brick short": dict(records=lambda r: r[:-1]),
        "records of another degree": dict(sh_degree=np.int32(2)), "brick 5": dict(brick=np.int32(5)),
        "table of another brick size": dict(brick=np.int32(4)), "short bits": dict(words=lambda w: w[:-1]),
        "entry = n_bricks": dict(brick_of=_set(n - 1, n)), "entry -2": dict(brick_of=_set(0, -2)), "repeated slot": dict(brick_of=_set(4, 3)),
        "hi below lo": dict(hi=np.asarray(LO, dtype=np.float64)), "negative threshold": dict(sigma_threshold=np.float64(-1.0)),
    }

    def forbidden(*a, **k):
        raise AssertionError("a damaged file reached the upload")
    for what, change in damage.items():
        path = str(tmp_path / "damaged.npz")
        _file(path, **change)
        with pytest.raises(ValueError):
            baked.read_quantized_brick_file(path)
        with monkeypatch.context() as m:
            m.setattr(torch, "as_tensor", forbidden)
            with pytest.raises(ValueError):
                QuantizedBrickField.load(path, device="cpu")
            if "format" not in change:
                with pytest.raises(ValueError):
                    baked.load_field(path, device="cpu")
    # an unused exponent byte is never trusted: any value there is read without complaint
    path = str(tmp_path / "unused.npz")
    _file(path, exponents=_exp_byte(1, 3, 0x7F))
    assert baked.read_quantized_brick_file(path)["n_bricks"] == n
    # the missing-key message names the format (load_field hands a format-3 file without the new keys to this reader)
    path = str(tmp_path / "three.npz")
    _file(path, exponents=None, quant_bits=None)
    with pytest.raises(ValueError, match="format"):
        baked.load_field(path)


def test_python_surface_refuses():
    import torch
    from keras_nerf_amd import baked, baked_quant, baked_train
    from keras_nerf_amd.baked import BakedField, QuantizedBrickField
    from keras_nerf_amd.baked_pose import PoseOptimizer
    field = _host_field()[0]
    for bad in (4, 16, 0, 7, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match="bit"):
            field.quantize(bits=bad)
        with pytest.raises(ValueError, match="bit"):
            baked_quant.check_bits(bad)
    assert baked_quant.check_bits(8) == 8 and baked_quant.check_bits(np.int64(8)) == 8
    dense = BakedField(torch.zeros((27, 16), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), (3, 3, 3), (LO, HI), 0)
    with pytest.raises(ValueError, match="brick"):
        dense.quantize(brick=5)
    with pytest.raises(ValueError, match="bit"):
        dense.quantize(bits=4)
    for bad in (-1, 4, 2.0, None):
        with pytest.raises(ValueError, match="sh_degree"):
            baked.quantized_record_bytes(bad)
    with pytest.raises(ValueError):
        baked.quantize_bricks(np.zeros((2, 64, 32), dtype=np.uint8), 2)                 # records of degree 1
    with pytest.raises(ValueError):
        baked.dequantize_bricks(np.zeros((2, 64, 64), dtype=np.uint8), np.zeros(2, dtype=np.uint32), 2)
    with pytest.raises(ValueError):
        baked.dequantize_bricks(np.zeros((2, 64, 32), dtype=np.uint8), np.zeros(3, dtype=np.uint32), 2)
    qf, q, e, brick_of, words = _host_qfield()
    # the constructor
    rec, ex = qf._records, qf._exponents
    for args in ((rec[:, :, :16], ex), (rec, ex[:-1]), (rec, ex.to(torch.int64)), (rec.reshape(-1, 32), ex), (rec[:0], ex[:0])):
        with pytest.raises(ValueError):
            QuantizedBrickField(args[0], args[1], qf._brick_of, qf._words, RES, (LO, HI), 2, 4)
    with pytest.raises(ValueError):
        QuantizedBrickField(rec, ex, qf._brick_of, qf._words, RES, (LO, HI), 2, 8)
    # what leads back through dequantize()
    o, d = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    t = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match=r"dequantize\(\)"):
        baked_train.brick_optimizer(qf, 1e-2, 1e-2)
    with pytest.raises(ValueError, match=r"dequantize\(\)"):
        qf.ray_gradients(o, d, 0.0, 6.0, t)
    with pytest.raises(ValueError, match=r"dequantize\(\)"):
        qf.optimizer(1e-2, 1e-2)
    with pytest.raises(ValueError, match=r"dequantize\(\)"):
        qf.resample(9)
    pose = PoseOptimizer.__new__(PoseOptimizer)                            # accumulate refuses the field before it looks at itself
    with pytest.raises(ValueError, match=r"dequantize\(\)"):
        pose.accumulate(qf, o, d, 0.0, 6.0, t, np.zeros(4, np.int32))
    # render: refused on the host, before the library is asked (the tensors here are not even on a device)
    for bad in (dict(step=-1.0), dict(step=0.0), dict(step=float("nan")), dict(termination=1.0), dict(termination=-0.1),
                dict(outputs=("rgb",)), dict(outputs=()), dict(outputs=("image", "image")), dict(lanes_per_ray=4), dict(lanes_per_ray=3)):
        with pytest.raises(ValueError):
            qf.render(o, d, 0.0, 6.0, **bad)
    q3 = _host_qfield(3, 8)[0]
    q1 = _host_qfield(1, 8)[0]
    for f, bad in ((q3, 2), (q1, 2), (q1, 4), (_host_qfield(0, 4)[0], 2)):
        with pytest.raises(ValueError, match="lanes_per_ray"):
            f.render(o, d, 0.0, 6.0, lanes_per_ray=bad)


def test_bake_refuses_quantize_without_bricks():
    """decided before the network is looked at"""
    from keras_nerf_amd.baked import bake
    with pytest.raises(ValueError, match="bricks"):
        bake(None, resolution=8, quantize=True)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID decided on the host: no device is needed and no pointer is dereferenced"""
    import ctypes as C
    from keras_nerf_amd import _lib
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    p, p2, p3 = C.c_void_p(1 << 20), C.c_void_p(1 << 30), C.c_void_p(1 << 40)

    def bricks(res=(19, 17, 12), degree=2, lo=LO, hi=HI, records=p, brick_of=p, bits=p, log2=3, n_bricks=11, **_):
        return _lib.KnerfBakedBricks(records, brick_of, bits, (C.c_int32 * 3)(*res), degree, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), log2,
                                     n_bricks)

    def render(null=False, exponents=p2, o=p, d=p, near=None, far=None, near_all=2.0, far_all=6.0, n_rays=0, step=0.02, eps=0.0,
               flags=_lib.BAKED_SKIP_EMPTY, image=p, depth=None, opacity=None, stats=None, **kw):
        f = _lib.KnerfBakedQBricks(bricks(**kw), exponents)
        return lib.knerf_baked_render_qbricks(None, None if null else C.byref(f), o, d, near, far, near_all, far_all, n_rays, step, eps,
                                              flags, image, depth, opacity, stats)

    lanes = lambda n: _lib.BAKED_SKIP_EMPTY | (n << _lib.BAKED_LANES_SHIFT)
    # good arguments and no ray: KNERF_OK without a launch
    assert render() == 0 and render(log2=2, n_bricks=75) == 0 and render(n_bricks=18) == 0 and render(n_bricks=1) == 0
    assert render(bits=None, flags=0) == 0 and render(flags=lanes(1)) == 0 and render(flags=lanes(2)) == 0
    assert render(degree=3, flags=lanes(4)) == 0 and render(degree=1, flags=lanes(1)) == 0 and render(degree=0) == 0
    nan, inf = float("nan"), float("inf")
    field_errors = (
        dict(records=None), dict(degree=-1), dict(degree=4), dict(res=(1, 17, 12)), dict(res=(19, 1026, 12)), dict(res=(19, 17, 0)),
        dict(hi=(1.0, -0.8, 0.7)), dict(lo=(nan, -0.8, -0.6)), dict(hi=(inf, 0.8, 0.7)), dict(log2=0), dict(log2=1), dict(log2=4),
        dict(log2=-3), dict(n_bricks=0), dict(n_bricks=19), dict(log2=2, n_bricks=76), dict(n_bricks=1 << 40), dict(n_bricks=(1 << 64) - 1),
        dict(res=(1025, 1025, 1025), degree=3, log2=2, n_bricks=(1 << 40) // (64 * 112) + 1))
    for bad in field_errors + (
            dict(null=True), dict(exponents=None), dict(brick_of=None), dict(o=None), dict(d=None), dict(image=None), dict(step=0.0),
            dict(step=-0.02), dict(step=nan), dict(step=inf), dict(eps=1.0), dict(eps=-0.1), dict(eps=nan), dict(flags=4),
            dict(flags=1 << 12), dict(flags=lanes(4)), dict(flags=lanes(3)), dict(degree=1, flags=lanes(2)), dict(degree=1, flags=lanes(4)),
            dict(degree=3, flags=lanes(2)), dict(degree=0, flags=lanes(2)), dict(bits=None), dict(n_rays=1 << 36), dict(near_all=nan),
            dict(far_all=inf)):
        assert render(**bad) == INV, bad

    # the codec: KNERF_OK cannot be shown without a launch (n_bricks >= 1), the refusals can
    def quantize(null=False, dst=p2, exps=p3, **kw):
        f = bricks(**kw)
        return lib.knerf_baked_quantize_bricks(None, None if null else C.byref(f), dst, exps)

    def dequantize(null=False, exponents=p3, dst=p2, **kw):
        f = _lib.KnerfBakedQBricks(bricks(**kw), exponents)
        return lib.knerf_baked_dequantize_bricks(None, None if null else C.byref(f), dst)

    src_bytes, q_bytes = 11 * 512 * 64, 11 * 512 * 32
    at = lambda x: C.c_void_p(x)
    for bad in field_errors + (dict(null=True), dict(dst=None), dict(exps=None),
                               # destination records inside, across the end of, and around the source; exponents inside the source / the destination
                               dict(dst=at((1 << 20) + 64)), dict(dst=at((1 << 20) + src_bytes - 1)), dict(dst=at((1 << 20) - q_bytes + 1)),
                               dict(dst=p), dict(exps=at((1 << 20) + 128)), dict(exps=at((1 << 30) + 4))):
        assert quantize(**bad) == INV, bad
    for bad in field_errors + (dict(null=True), dict(dst=None), dict(exponents=None),
                               dict(dst=at((1 << 20) + 32)), dict(dst=at((1 << 20) + q_bytes - 1)), dict(dst=at((1 << 20) - src_bytes + 1)),
                               dict(dst=p), dict(dst=at((1 << 40) - 16))):
        assert dequantize(**bad) == INV, bad
