"""The brick storage of a baked field on the GPU (keras_nerf_amd/baked.py BrickBakedField, csrc/baked.hip): renders that are
bit-identical to the dense field's for every degree, kernel variant, skipping on / off, background and brick size; compact / to_dense
against tests/baked_bricks_reference.py; persistence; baking straight into bricks.  The conditions are stated in
tests/README_baked_bricks.md.  No test feeds the kernel a damaged table: its range guard is checked by reading."""
import numpy as np
import pytest
import torch

from tests import baked_bricks_reference as B
from tests import baked_reference as R
from tests.test_baked_bricks_host import BRICKS, HI, LO, RES, lattice, scene
from tests.test_gpu_baked import N_RAYS, STEP, VARIANTS, rays  # noqa: F401 -- the ray set of the dense tests (a fixture), over the same box

pytestmark = pytest.mark.gpu

OUT = ("image", "depth", "opacity")
_fields = {}


def _dense(degree):
    """the dense field of the test lattice, built once per degree and never changed"""
    from keras_nerf_amd.baked import BakedField
    if degree not in _fields:
        sigma, co = lattice(degree)
        _fields[degree] = BakedField.from_arrays(sigma, co, (LO, HI))
    return _fields[degree]


def _render(field, rays, **kw):
    out = field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, stats=True, **kw)
    torch.cuda.synchronize()
    return out


def _same(a, b, what):
    for k in OUT:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))
    assert torch.equal(a["stats"], b["stats"]), (what, a["stats"].tolist(), b["stats"].tolist())


def _samples_in_absent_bricks(rays, brick_of, b):
    """per ray: the number of samples inside the box (float64 positions) with a corner of their cell in an absent brick"""
    lo, hi, res = np.array(LO, np.float32).astype(np.float64), np.array(HI, np.float32).astype(np.float64), np.array(RES)
    hits = np.zeros(N_RAYS, dtype=np.int64)
    for r in range(N_RAYS):
        S = int(np.ceil((float(rays["far"][r]) - float(rays["near"][r])) / STEP))
        t = float(rays["near"][r]) + (np.arange(S) + 0.5) * STEP
        p = rays["o"][r].astype(np.float64) + rays["d"][r].astype(np.float64) * t[:, None]
        u = (p - lo) / (hi - lo) * (res - 1)
        inside = np.all((u >= 0) & (u <= res - 1), axis=1)
        cell = np.minimum(np.floor(u[inside]), res - 2).astype(np.int64)
        absent = np.zeros(len(cell), dtype=bool)
        for i in (0, 1):
            for j in (0, 1):
                for k in (0, 1):
                    absent |= brick_of[(cell[:, 0] + i) // b, (cell[:, 1] + j) // b, (cell[:, 2] + k) // b] < 0
        hits[r] = int(absent.sum())
    return hits


@pytest.mark.parametrize("b", BRICKS)
def test_inputs_have_what_the_tests_need(b, rays):
    sigma, co, rec, occ, brick_of, n = scene(2, b)
    assert (brick_of < 0).any() and (brick_of >= 0).any() and B.partial_edge_bricks(brick_of, RES, b).any() and occ[7, 7, 7]
    x, y, z = np.meshgrid(*(np.arange(r) for r in RES), indexing="ij")
    absent = brick_of[x // b, y // b, z // b] < 0
    assert (sigma[absent] == 0).all() and (co[absent].astype(np.float32) != 0).mean() > 0.99           # non-zero colour there
    hits = _samples_in_absent_bricks(rays, brick_of, b)
    assert (hits > 0).any(), hits
    # the dense field of the test is this lattice, bit for bit
    field = _dense(2)
    assert np.array_equal(field._records.cpu().numpy(), rec) and np.array_equal(field.occupied.cpu().numpy(), occ)


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_renders_are_bit_identical_to_the_dense_field(degree, b, rays):
    """image, depth, opacity and stats of BrickBakedField.render equal BakedField.render's bits for every kernel variant, skipping on
    and off, both backgrounds, and once more with termination.  With skip_empty=False samples in empty cells are fetched: their corners
    in absent bricks read as zero where the dense table holds non-zero coefficients, and sigma = 0 gives w = 0 either way."""
    dense = _dense(degree)
    field = dense.compact(b)
    assert field.brick == b and field.n_bricks == scene(degree, b)[5]
    fetched = {}
    for lanes in VARIANTS[degree]:
        for skip in (True, False):
            for white in (False, True):
                for eps in (0.0, 1e-2):
                    kw = dict(lanes_per_ray=lanes, skip_empty=skip, white_background=white, termination=eps)
                    a, c = _render(dense, rays, **kw), _render(field, rays, **kw)
                    _same(a, c, (degree, b, kw))
                    fetched[(skip, eps)] = int(c["stats"][0])
    assert 0 < fetched[(True, 0.0)] < fetched[(False, 0.0)] and fetched[(True, 1e-2)] < fetched[(True, 0.0)]     # both knobs did something
    out = field.render(rays["o"], rays["d"], 0.0, 6.0, outputs=("opacity",))
    assert sorted(out) == ["opacity"] and torch.equal(out["opacity"], dense.render(rays["o"], rays["d"], 0.0, 6.0, outputs=("opacity",))["opacity"])
    assert float(out["opacity"].max()) > 0.5


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 3])
def test_compact_and_to_dense_against_the_reference(degree, b):
    _, _, rec, occ, brick_of, n = scene(degree, b)
    dense = _dense(degree)
    field = dense.compact(b)
    want = B.bricks_from_dense(rec, brick_of, n, RES, b)
    assert field.n_bricks == n and np.array_equal(field.brick_of.cpu().numpy(), brick_of) and field.brick_of.dtype == torch.int32
    assert np.array_equal(field._records.cpu().numpy(), want)
    assert torch.equal(field._words, dense._words) and np.array_equal(field.occupied.cpu().numpy(), occ)
    assert field.resolution == RES and field.bounds == (LO, HI) and field.sh_degree == degree and field.device == dense.device
    assert field.nbytes == want.nbytes + brick_of.nbytes + 4 * dense._words.numel() and field.cell_size == dense.cell_size
    back = field.to_dense()
    assert np.array_equal(back._records.cpu().numpy(), B.dense_from_bricks(want, brick_of, RES, b)) and torch.equal(back._words, dense._words)
    assert back.resolution == RES and back.bounds == (LO, HI) and back.sh_degree == degree
    assert torch.equal(back.compact(b)._records, field._records)
    assert np.array_equal(dense._records.cpu().numpy(), rec)               # compact leaves the dense field as it is


@pytest.mark.parametrize("b", BRICKS)
def test_save_load_render(b, tmp_path, rays):
    from keras_nerf_amd import baked
    from keras_nerf_amd.baked import BakedField, BrickBakedField
    dense = _dense(2)
    field = dense.compact(b)
    path = str(tmp_path / "scene")
    field.save(path)
    n = scene(2, b)[5]
    with np.load(path) as z:
        assert int(z["format"]) == 2 and z["records"].shape == (n, b ** 3, 64) and int(z["brick"]) == b
    again = BrickBakedField.load(path)
    assert again.brick == b and again.n_bricks == n and again.resolution == RES and again.bounds == field.bounds and again.sh_degree == 2
    assert torch.equal(again._records, field._records) and torch.equal(again.brick_of, field.brick_of) and torch.equal(again._words, field._words)
    for kw in (dict(), dict(skip_empty=False, white_background=True)):
        _same(_render(dense, rays, **kw), _render(again, rays, **kw), (b, kw))
    assert isinstance(baked.load_field(path), BrickBakedField)
    with pytest.raises(ValueError, match="format"):
        BakedField.load(path)
    one = str(tmp_path / "dense")
    dense.save(one)
    assert isinstance(baked.load_field(one), BakedField)
    with pytest.raises(ValueError):
        BrickBakedField.load(one)


def test_bake_into_bricks_equals_bake_then_compact():
    """NeRF.bake(bricks=b) against bake().compact(b), byte for byte, with the network, lattice and slabs of
    test_gpu_baked.test_bake_against_the_network (eleven slabs); bricks=None is the dense bake"""
    from keras_nerf_amd.baked import BakedField, BrickBakedField, bake
    from tests.test_gpu_query import _nerf
    nerf, _ = _nerf()
    res, bounds = (12, 10, 9), ((-1.5,) * 3, (1.5,) * 3)
    tau = float(np.quantile(nerf.density_grid(res, bounds).cpu().numpy(), 0.6))
    kw = dict(resolution=res, bounds=bounds, sh_degree=2, n_directions=32, sigma_threshold=tau)
    dense = bake(nerf, slab_bytes=24 * 9 * 100, **kw)
    plain = nerf.bake(**kw)
    none = nerf.bake(bricks=None, **kw)
    assert type(dense) is BakedField and type(none) is BakedField
    assert torch.equal(none._records, plain._records) and torch.equal(none._words, plain._words) and torch.equal(none._records, dense._records)
    occ = dense.occupied.cpu().numpy()
    assert occ.any() and not occ.all() and int(R.touched_points(occ).sum()) > 1000
    for b in BRICKS:
        want = dense.compact(b)
        brick_of, n = B.brick_table(occ, res, b)
        assert want.n_bricks == n and np.array_equal(want.brick_of.cpu().numpy(), brick_of)
        for got in (bake(nerf, slab_bytes=24 * 9 * 100, bricks=b, **kw), nerf.bake(bricks=b, **kw)):
            assert type(got) is BrickBakedField and got.brick == b and got.n_bricks == n and got.sigma_threshold == tau
            assert torch.equal(got._records, want._records) and torch.equal(got.brick_of, want.brick_of) and torch.equal(got._words, want._words)
            assert got._records.any() and got._bake_sigma is None
        o = np.array([[0.0, 0.0, 4.0]] * 5, dtype=np.float32); d = np.array([[0.0, 0.0, -1.0]] * 5, dtype=np.float32)
        o[:, 0] = np.linspace(-1.0, 1.0, 5)
        x, y = dense.render(o, d, 2.0, 6.0, stats=True), got.render(o, d, 2.0, 6.0, stats=True)
        assert all(torch.equal(x[k], y[k]) for k in OUT + ("stats",)) and float(y["opacity"].max()) > 0
    with pytest.raises(ValueError, match="brick"):
        nerf.bake(bricks=16, **kw)
