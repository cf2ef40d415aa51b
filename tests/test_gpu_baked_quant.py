"""The 8-bit codec of brick baked fields on the GPU (keras_nerf_amd/baked_quant.py QuantizedBrickField, csrc/baked_quant.hip): the codec
launches against tests/baked_quant_reference.py byte for byte; the one-ray-per-lane render of the quantised bricks bit-identical to the
brick render of the dequantised field; every variant against the fp64 marcher on the dequantised arrays; exact skipping; padding that
is never trusted; persistence; baking straight into a quantised field.  The conditions are stated in tests/README_baked_quant.md.  No
test feeds a kernel a damaged table or an exponent out of range: the range guards are checked by reading.

Measured on an MI355X (largest deviation from the fp64 marcher over the 150 rays, every degree, brick size and kernel variant within
these): image 4.5e-7 (bound 1e-5), depth 1.1e-6 (bound 2.1e-4), opacity 3.7e-7 (bound 1e-5); the quantised image moves away from the
unquantised brick field's by at most 2.26e-3 (b = 8) / 2.93e-3 (b = 4) at degree 2.  The tests print the figures of the run."""
import numpy as np
import pytest
import torch

from tests import baked_bricks_reference as B
from tests import baked_quant_reference as Q
from tests import baked_reference as R
from tests.test_baked_bricks_host import BRICKS, HI, LO, RES
from tests.test_baked_quant_host import qscene
from tests.test_gpu_baked import N_RAYS, STEP, rays  # noqa: F401 -- the ray set of the dense tests (a fixture), over the same box

pytestmark = pytest.mark.gpu

OUT = ("image", "depth", "opacity")
QVARIANTS = {0: (0, 1), 1: (0, 1), 2: (0, 1, 2), 3: (0, 1, 4)}        # lanes_per_ray values per degree (0: the default)
_fields, _refs = {}, {}


def _bricks(degree, b):
    """the unquantised brick field of the quantisation test lattice, built once per case and never changed"""
    from keras_nerf_amd.baked import BakedField
    if (degree, b) not in _fields:
        sigma, co = qscene(degree, b)[:2]
        _fields[(degree, b)] = BakedField.from_arrays(sigma, co, (LO, HI)).compact(b)
    return _fields[(degree, b)]


def _dequantised_arrays(degree, b):
    """(sigma [RES], coefficients [RES, K, 3] fp16) of the dequantised field as dense arrays, from the NumPy references alone"""
    from keras_nerf_amd.baked import unpack_records
    bricks, brick_of = qscene(degree, b)[5], qscene(degree, b)[3]
    q, e = Q.quantize(bricks, degree)
    dense = B.dense_from_bricks(Q.dequantize(q, e, degree), brick_of, RES, b)
    sg, co = unpack_records(dense, degree)
    return sg.reshape(RES), co.reshape(RES + co.shape[1:])


def _reference(degree, b, rays):
    """the fp64 marcher on the dequantised arrays and the fp32 marcher's own deviation from it, computed once per case and shared; the
    bound of tests/test_gpu_baked.py: max(1e-5 x scale, 4 x that deviation) per output"""
    if (degree, b) not in _refs:
        sigma, co = _dequantised_arrays(degree, b)
        args = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP)
        r64 = R.march(*args, termination=0.0, dtype=np.float64)
        r32 = R.march(*args, termination=0.0, dtype=np.float32)
        scale = (1.0, float(rays["far"].max()), 1.0)
        bound = [max(1e-5 * s, 4.0 * float(np.abs(a.astype(np.float64) - c).max())) for a, c, s in zip(r32, r64, scale)]
        _refs[(degree, b)] = (r64, bound)
    return _refs[(degree, b)]


def _render(field, rays, **kw):
    out = field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, stats=True, **kw)
    torch.cuda.synchronize()
    return out


def _same(a, b, what):
    for k in OUT:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))
    assert torch.equal(a["stats"], b["stats"]), (what, a["stats"].tolist(), b["stats"].tolist())


def test_inputs_have_what_the_tests_need(rays):
    """so that clamping, equal exponents or rays that miss cannot hide a decode error"""
    bricks, brick_of = qscene(2, 8)[5], qscene(2, 8)[3]
    q, e = Q.quantize(bricks, 2)
    ex = Q.exponents_of(e, 2)
    corners = {tuple(ex[brick_of[x // 8, y // 8, z // 8]]) for x in (7, 8) for y in (7, 8) for z in (7, 8)}
    assert len(corners) >= 3, corners
    assert any(len(set(row)) > 1 for row in ex.tolist())                   # an exponent word with two different band bytes
    qi = q[:, :, 4:31].view(np.int8)
    assert np.abs(qi.astype(np.int64)).max() >= 126                        # the codes use their whole range
    for b in BRICKS:
        (img, dep, opa), _ = _reference(2, b, rays)
        hit = opa > 0.05
        unclamped = hit & ((img > 0.02) & (img < 0.98)).all(axis=1)
        assert hit.sum() >= 25 and unclamped.sum() >= 25, (b, int(hit.sum()), int(unclamped.sum()))
        # the field under test is this lattice, bit for bit
        assert np.array_equal(_bricks(2, b)._records.cpu().numpy(), qscene(2, b)[5])


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_codec_against_the_reference(degree, b):
    from keras_nerf_amd.baked import BrickBakedField, QuantizedBrickField
    src = _bricks(degree, b)
    bricks = qscene(degree, b)[5]
    before = src._records.clone()
    want_q, want_e = Q.quantize(bricks, degree)
    q = src.quantize()
    assert type(q) is QuantizedBrickField and q.brick == b and q.n_bricks == src.n_bricks and q.sh_degree == degree
    assert q.resolution == RES and q.bounds == (LO, HI) and q.sigma_threshold == src.sigma_threshold and q.device == src.device
    assert np.array_equal(q._records.cpu().numpy(), want_q)
    assert np.array_equal(q.exponents.cpu().numpy().view(np.uint32), want_e)
    assert torch.equal(q.brick_of, src.brick_of) and torch.equal(q._words, src._words) and torch.equal(q.occupied, src.occupied)
    assert q.nbytes == want_q.nbytes + want_e.nbytes + 4 * src.brick_of.numel() + 4 * src._words.numel() and q.cell_size == src.cell_size
    assert torch.equal(src._records, before)                               # the source is left as it is
    d = q.dequantize()
    assert type(d) is BrickBakedField and d.brick == b and d.n_bricks == src.n_bricks
    assert np.array_equal(d._records.cpu().numpy(), Q.dequantize(want_q, want_e, degree))
    assert torch.equal(d.brick_of, src.brick_of) and torch.equal(d._words, src._words)
    again = d.quantize()
    assert torch.equal(again._records, q._records) and torch.equal(again.exponents, q.exponents)
    assert torch.equal(q.to_dense()._records, d.to_dense()._records)
    # the dense field's shorthand
    short = src.to_dense().quantize(brick=b)
    assert torch.equal(short._records, q._records) and torch.equal(short.exponents, q.exponents)
    # a second launch writes the same bytes
    twice = src.quantize()
    assert torch.equal(twice._records, q._records) and torch.equal(twice.exponents, q.exponents)


def test_codec_on_special_values():
    """NaN, +-inf, 65504, subnormals, -0, an all-zero band and the two maxima around 127 x 2^e through the kernels: the bytes of the
    reference"""
    from keras_nerf_amd.baked import BrickBakedField
    from tests.test_baked_quant_host import _special_bricks
    rec, at, _ = _special_bricks()
    n = rec.shape[0]
    table = torch.full((3, 3, 3), -1, dtype=torch.int32)
    table.reshape(-1)[:n] = torch.arange(n, dtype=torch.int32)
    field = BrickBakedField(torch.as_tensor(rec).cuda(), table.cuda(), torch.zeros(42, dtype=torch.int32).cuda(), (12, 12, 12), (LO, HI), 2, 4)
    q = field.quantize()
    want_q, want_e = Q.quantize(rec, 2)
    assert np.array_equal(q._records.cpu().numpy(), want_q) and np.array_equal(q.exponents.cpu().numpy().view(np.uint32), want_e)
    assert np.array_equal(q.dequantize()._records.cpu().numpy(), Q.dequantize(want_q, want_e, 2))


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_one_ray_per_lane_is_bit_identical_to_the_dequantised_field(degree, b, rays):
    """image, depth, opacity and stats of QuantizedBrickField.render(lanes_per_ray=1) equal BrickBakedField.render(lanes_per_ray=1) of
    dequantize() bit for bit, with skipping on and off, both backgrounds, and with termination"""
    q = _bricks(degree, b).quantize()
    d = q.dequantize()
    fetched = {}
    for skip in (True, False):
        for white in (False, True):
            for eps in (0.0, 1e-2):
                kw = dict(lanes_per_ray=1, skip_empty=skip, white_background=white, termination=eps)
                a, c = _render(d, rays, **kw), _render(q, rays, **kw)
                _same(a, c, (degree, b, kw))
                fetched[(skip, eps)] = int(c["stats"][0])
    assert 0 < fetched[(True, 0.0)] < fetched[(False, 0.0)] and fetched[(True, 1e-2)] < fetched[(True, 0.0)]     # both knobs did something
    out = q.render(rays["o"], rays["d"], 0.0, 6.0, outputs=("opacity",), lanes_per_ray=1)
    want = d.render(rays["o"], rays["d"], 0.0, 6.0, outputs=("opacity",), lanes_per_ray=1)
    assert sorted(out) == ["opacity"] and torch.equal(out["opacity"], want["opacity"]) and float(out["opacity"].max()) > 0.5


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_every_variant_matches_the_fp64_marcher(degree, b, rays):
    """every kernel variant of the degree, the default included, against the fp64 marcher on the dequantised dense arrays; bound per
    output: max(1e-5 x scale, 4 x the fp32 reference's own deviation from the fp64 reference).  The stats are those of the unquantised
    brick field exactly: sigma and the bits are untouched, so the same samples are fetched."""
    (img, dep, opa), bound = _reference(degree, b, rays)
    src = _bricks(degree, b)
    q = src.quantize()
    want_stats = _render(src, rays)["stats"]
    for lanes in QVARIANTS[degree]:
        out = _render(q, rays, lanes_per_ray=lanes)
        assert out["image"].shape == (N_RAYS, 3) and out["depth"].shape == (N_RAYS,) and out["opacity"].shape == (N_RAYS,)
        errs = [float(np.abs(out[k].cpu().numpy().astype(np.float64) - ref).max()) for k, ref in
                (("image", img), ("depth", dep), ("opacity", opa))]
        print(f"degree {degree} b {b} lanes {lanes}: max |image, depth, opacity - fp64| = {errs}, bounds {bound}")
        for e, bd, k in zip(errs, bound, OUT):
            assert e <= bd, (degree, b, lanes, k, e, bd)
        assert torch.equal(out["stats"], want_stats), (degree, b, lanes, out["stats"].tolist(), want_stats.tolist())
        assert 0 < int(out["stats"][0]) < int(out["stats"][1])


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_skipping_is_exact_in_every_variant(degree, rays):
    for b in BRICKS:
        q = _bricks(degree, b).quantize()
        for lanes in QVARIANTS[degree]:
            for white in (False, True):
                a = _render(q, rays, lanes_per_ray=lanes, skip_empty=True, white_background=white)
                c = _render(q, rays, lanes_per_ray=lanes, skip_empty=False, white_background=white)
                for k in OUT:
                    assert torch.equal(a[k], c[k]), (degree, b, lanes, k)
                sa, sc = a["stats"].cpu().numpy(), c["stats"].cpu().numpy()
                assert sa[0] < sc[0] <= sc[1] and sa[1] == sc[1], (sa, sc)


@pytest.mark.parametrize("b", BRICKS)
def test_the_quantisation_is_real(b, rays):
    """the image of the quantised field differs from the unquantised brick field's on a hitting ray; how far is printed, not bounded.
    Measured on an MI355X, degree 2: 2.26e-3 (b = 8), 2.93e-3 (b = 4); all 33 hitting rays differ."""
    src = _bricks(2, b)
    a, c = _render(src, rays, lanes_per_ray=1), _render(src.quantize(), rays, lanes_per_ray=1)
    hit = (a["opacity"] > 0.05)
    diff = (a["image"] - c["image"]).abs().max(dim=1).values
    print(f"b {b}: largest |image(quantised) - image(bricks)| = {float(diff.max())}, mean {float(diff[hit].mean())}, "
          f"{int((diff[hit] > 0).sum())} of {int(hit.sum())} hitting rays differ")
    assert int(hit.sum()) >= 25 and bool((diff[hit] > 0).any())
    assert torch.equal(a["opacity"], c["opacity"]) and torch.equal(a["depth"], c["depth"])         # density is not quantised


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_padding_is_never_trusted(degree, rays):
    """record padding and the exponent bytes of bands above the degree filled with 0xFF: every variant renders the bits of the clean
    field (degree 1 has no record padding, degree 3 no unused exponent byte)"""
    from keras_nerf_amd.baked import QuantizedBrickField
    K = (degree + 1) ** 2
    for b in BRICKS:
        q = _bricks(degree, b).quantize()
        rec, ex = q._records.clone(), q.exponents.clone()
        rec[:, :, 4 + 3 * K:] = 0xFF
        if degree < 3:
            ex |= torch.tensor(-1 << (8 * (degree + 1)), dtype=torch.int32, device=ex.device)
        assert not torch.equal(rec, q._records) or degree == 1
        assert not torch.equal(ex, q.exponents) or degree == 3
        dirty = QuantizedBrickField(rec, ex, q.brick_of, q._words, RES, (LO, HI), degree, b)
        for lanes in QVARIANTS[degree]:
            for kw in (dict(), dict(skip_empty=False, white_background=True)):
                _same(_render(q, rays, lanes_per_ray=lanes, **kw), _render(dirty, rays, lanes_per_ray=lanes, **kw), (degree, b, lanes, kw))
        # the decoder does not read them either
        assert torch.equal(dirty.dequantize()._records, q.dequantize()._records)


@pytest.mark.parametrize("b", BRICKS)
def test_save_load_render(b, tmp_path, rays):
    from keras_nerf_amd import baked
    from keras_nerf_amd.baked import BrickBakedField, QuantizedBrickField
    q = _bricks(2, b).quantize()
    path = str(tmp_path / "scene")
    q.save(path)
    with np.load(path) as z:
        assert int(z["format"]) == 3 and int(z["quant_bits"]) == 8 and z["records"].shape == (q.n_bricks, b ** 3, 32)
        assert z["exponents"].dtype == np.uint32 and z["exponents"].shape == (q.n_bricks,)
    again = baked.load_field(path)
    assert type(again) is QuantizedBrickField and again.brick == b and again.n_bricks == q.n_bricks and again.bounds == q.bounds
    assert torch.equal(again._records, q._records) and torch.equal(again.exponents, q.exponents)
    assert torch.equal(again.brick_of, q.brick_of) and torch.equal(again._words, q._words)
    for kw in (dict(), dict(lanes_per_ray=1, skip_empty=False, white_background=True)):
        _same(_render(q, rays, **kw), _render(again, rays, **kw), (b, kw))
    with pytest.raises(ValueError, match="format"):
        BrickBakedField.load(path)


def test_bake_quantized_equals_bake_then_quantize():
    """NeRF.bake(bricks=8, quantize=True) against NeRF.bake(bricks=8).quantize(), byte for byte, with the network and lattice of
    test_gpu_baked_bricks.test_bake_into_bricks_equals_bake_then_compact"""
    from keras_nerf_amd.baked import BakedField, BrickBakedField, QuantizedBrickField
    from tests.test_gpu_query import _nerf
    nerf, _ = _nerf()
    res, bounds = (12, 10, 9), ((-1.5,) * 3, (1.5,) * 3)
    tau = float(np.quantile(nerf.density_grid(res, bounds).cpu().numpy(), 0.6))
    kw = dict(resolution=res, bounds=bounds, sh_degree=2, n_directions=32, sigma_threshold=tau)
    plain = nerf.bake(bricks=8, **kw)
    want = plain.quantize()
    got = nerf.bake(bricks=8, quantize=True, **kw)
    assert type(plain) is BrickBakedField and type(got) is QuantizedBrickField and got.sigma_threshold == tau and got.brick == 8
    assert torch.equal(got._records, want._records) and torch.equal(got.exponents, want.exponents)
    assert torch.equal(got.brick_of, plain.brick_of) and torch.equal(got._words, plain._words) and got._records.any()
    assert np.array_equal(want._records.cpu().numpy(), Q.quantize(plain._records.cpu().numpy(), 2)[0])
    # the defaults are what they were
    assert type(nerf.bake(**kw)) is BakedField and type(nerf.bake(bricks=8, quantize=False, **kw)) is BrickBakedField
    with pytest.raises(ValueError, match="bricks"):
        nerf.bake(quantize=True, **kw)
    o = np.array([[0.0, 0.0, 4.0]] * 5, dtype=np.float32); d = np.array([[0.0, 0.0, -1.0]] * 5, dtype=np.float32)
    o[:, 0] = np.linspace(-1.0, 1.0, 5)
    x, y = want.dequantize().render(o, d, 2.0, 6.0, stats=True, lanes_per_ray=1), got.render(o, d, 2.0, 6.0, stats=True, lanes_per_ray=1)
    assert all(torch.equal(x[k], y[k]) for k in OUT + ("stats",)) and float(y["opacity"].max()) > 0
