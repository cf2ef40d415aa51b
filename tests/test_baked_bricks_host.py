"""The brick storage of a baked field, the parts that need no GPU: the package's NumPy mirrors of the format (keras_nerf_amd/baked.py
brick_table, bricks_from_dense, dense_from_bricks) against tests/baked_bricks_reference.py, the round trip, the field without an
occupied cell, the host-side reader of format-2 files, the argument checks of the Python surface and of knerf_baked_render_bricks.
Every condition is stated in tests/README_baked_bricks.md."""
import numpy as np
import pytest

from tests import baked_bricks_reference as B
from tests import baked_reference as R

RES = (19, 17, 12)                      # 19 = 2 x 8 + 3, 17 = 2 x 8 + 1 = 4 x 4 + 1, 12 = 8 + 4: partial edge bricks for both brick sizes
LO, HI = (-1.0, -0.8, -0.6), (1.0, 0.8, 0.7)
BRICKS = (4, 8)


def lattice(degree, seed=0):
    """random coefficients at EVERY lattice point, sigma > 0 only in two separated blobs: points 6..9 on every axis (so cell (7, 7, 7)
    is occupied and its 8 corners lie in 8 different bricks of 8^3) and points (16..17, 14..15, 2..3) next to the +x / +y faces"""
    rng = np.random.default_rng(300 + seed)
    sigma = np.zeros(RES, dtype=np.float32)
    sigma[6:10, 6:10, 6:10] = rng.uniform(5.0, 30.0, (4, 4, 4)).astype(np.float32)
    sigma[16:18, 14:16, 2:4] = rng.uniform(5.0, 30.0, (2, 2, 2)).astype(np.float32)
    K = (degree + 1) ** 2
    co = (rng.standard_normal(RES + (K, 3)) * 0.6).astype(np.float16)
    co[..., 0, :] += np.float16(1.5)
    return sigma, co


def scene(degree, b):
    """(sigma, coefficients, dense records, occupied cells, brick_of, n_bricks) of the test lattice, all from the NumPy references"""
    from tests import baked_grow_reference as G
    sigma, co = lattice(degree)
    occ = R.occupied_cells(sigma)
    brick_of, n = B.brick_table(occ, RES, b)
    return sigma, co, G.pack(sigma, co, degree), occ, brick_of, n


@pytest.mark.parametrize("b", BRICKS)
def test_the_test_lattice_has_what_the_tests_need(b):
    _, _, _, occ, brick_of, n = scene(2, b)
    assert occ[7, 7, 7] and (brick_of >= 0).any() and (brick_of < 0).any() and n == int((brick_of >= 0).sum())
    assert B.partial_edge_bricks(brick_of, RES, b).any()
    assert n == {4: 16, 8: 11}[b]
    if b == 8:                                                             # the 8 corners of cell (7, 7, 7): 8 different bricks
        assert len({(x // 8, y // 8, z // 8) for x in (7, 8) for y in (7, 8) for z in (7, 8)}) == 8
    slots = brick_of.reshape(-1)[brick_of.reshape(-1) >= 0]
    assert np.array_equal(slots, np.arange(n))                             # ascending C order


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 3])
def test_package_mirrors_equal_the_reference(degree, b):
    from keras_nerf_amd import baked
    _, _, rec, occ, brick_of, n = scene(degree, b)
    got_of, got_n = baked.brick_table(occ, RES, b)
    assert got_of.dtype == np.int32 and np.array_equal(got_of, brick_of) and got_n == n and baked.brick_grid(RES, b) == brick_of.shape
    want = B.bricks_from_dense(rec, brick_of, n, RES, b)
    got = baked.bricks_from_dense(rec, brick_of, n, RES, b)
    assert got.dtype == np.uint8 and got.shape == (n, b ** 3, baked.record_bytes(degree)) and np.array_equal(got, want)
    assert np.array_equal(baked.dense_from_bricks(got, brick_of, RES, b), B.dense_from_bricks(want, brick_of, RES, b))
    # a record through the table is the dense record in a stored brick and zero in an absent one
    dense = rec.reshape(RES + (-1,))
    for x, y, z in ((7, 7, 7), (8, 8, 8), (18, 16, 3), (0, 0, 0), (18, 0, 11), (3, 16, 11)):
        stored = brick_of[x // b, y // b, z // b] >= 0
        assert np.array_equal(B.lookup(got, brick_of, b, x, y, z), dense[x, y, z] if stored else np.zeros_like(dense[x, y, z]))


@pytest.mark.parametrize("b", BRICKS)
def test_round_trip_keeps_stored_bricks_and_zeroes_the_rest(b):
    from keras_nerf_amd import baked
    _, _, rec, occ, brick_of, n = scene(2, b)
    bricks = baked.bricks_from_dense(rec, brick_of, n, RES, b)
    back = baked.dense_from_bricks(bricks, brick_of, RES, b).reshape(RES + (-1,))
    x, y, z = np.meshgrid(*(np.arange(r) for r in RES), indexing="ij")
    stored = brick_of[x // b, y // b, z // b] >= 0
    dense = rec.reshape(RES + (-1,))
    assert stored.any() and not stored.all()
    assert np.array_equal(back[stored], dense[stored]) and not back[~stored].any() and dense[~stored].any()
    # every touched point lies in a stored brick, and places past the lattice are zero records
    assert stored[R.touched_points(occ)].all()
    cube = bricks.reshape(n, b, b, b, -1)
    for (bx, by, bz), slot in np.ndenumerate(brick_of):
        if slot >= 0:
            nx, ny, nz = (min(b, r - c * b) for r, c in zip(RES, (bx, by, bz)))
            assert not cube[slot, nx:].any() and not cube[slot, :, ny:].any() and not cube[slot, :, :, nz:].any()
    # again: bricks of the round-tripped table are the same bricks
    assert np.array_equal(baked.bricks_from_dense(back.reshape(rec.shape), brick_of, n, RES, b), bricks)


@pytest.mark.parametrize("b", BRICKS)
def test_field_without_an_occupied_cell(b):
    from keras_nerf_amd import baked
    occ = np.zeros(tuple(r - 1 for r in RES), dtype=bool)
    rec = np.random.default_rng(1).integers(0, 255, (int(np.prod(RES)), 32), dtype=np.uint8)
    for mod in (B, baked):
        brick_of, n = mod.brick_table(occ, RES, b)
        assert n == 1 and (brick_of == -1).all()
        bricks = mod.bricks_from_dense(rec, brick_of, n, RES, b)
        assert bricks.shape == (1, b ** 3, 32) and not bricks.any()
        assert not mod.dense_from_bricks(bricks, brick_of, RES, b).any()


def _file(path, b=8, degree=1, **change):
    """a format-2 file written with NumPy from the references; `change` replaces or (value None) drops keys"""
    _, _, rec, occ, brick_of, n = scene(degree, b)
    from keras_nerf_amd.runtime import pack_occupancy
    data = dict(format=np.int32(2), records=B.bricks_from_dense(rec, brick_of, n, RES, b), brick_of=brick_of,
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


def _swap(i, j):
    def f(t):
        t = t.copy(); flat = t.reshape(-1)
        at = np.nonzero(flat >= 0)[0]
        flat[at[i]], flat[at[j]] = flat[at[j]], flat[at[i]]
        return t
    return f


def _set(i, value):
    def f(t):
        t = t.copy(); flat = t.reshape(-1)
        flat[np.nonzero(flat >= 0)[0][i]] = value
        return t
    return f


@pytest.mark.parametrize("b", BRICKS)
def test_reader_accepts_a_good_file(b, tmp_path):
    from keras_nerf_amd import baked
    path = str(tmp_path / "bricks")
    data = _file(path, b)
    got = baked.read_brick_file(path)
    assert got["brick"] == b and got["n_bricks"] == data["records"].shape[0] and got["resolution"] == RES and got["sh_degree"] == 1
    assert got["lo"] == LO and got["hi"] == HI and got["sigma_threshold"] == 0.0
    for k in ("records", "brick_of", "words"):
        assert isinstance(got[k], np.ndarray) and got[k].dtype == data[k].dtype and np.array_equal(got[k], data[k])


def test_reader_refuses_damaged_files(tmp_path, monkeypatch):
    """each kind of damage is a ValueError from the host-side reader; BrickBakedField.load goes through the same reader before it
    touches a device (torch.as_tensor / .to are never reached: the test forbids them)"""
    import torch
    from keras_nerf_amd import baked
    from keras_nerf_amd.baked import BakedField, BrickBakedField
    n = scene(1, 8)[5]
    damage = {
        "no brick table": dict(brick_of=None), "no records": dict(records=None), "no bits": dict(words=None), "no brick": dict(brick=None),
        "no format": dict(format=None), "no threshold": dict(sigma_threshold=None),
        "format 3": dict(format=np.int32(3)), "format 1": dict(format=np.int32(1)),
        "float records": dict(records=lambda r: r.astype(np.float32)), "flat records": dict(records=lambda r: r.reshape(-1, r.shape[2])),
        "a brick short": dict(records=lambda r: r[:-1]), "a brick more": dict(records=lambda r: np.concatenate([r, r[:1]])),
        "records of another degree": dict(sh_degree=np.int32(2)),
        "int64 table": dict(brick_of=lambda t: t.astype(np.int64)), "flat table": dict(brick_of=lambda t: t.reshape(-1)),
        "table of another brick size": dict(brick=np.int32(4)), "brick 5": dict(brick=np.int32(5)),
        "short bits": dict(words=lambda w: w[:-1]), "uint32 bits": dict(words=lambda w: w.astype(np.uint32)),
        "entry = n_bricks": dict(brick_of=_set(n - 1, n)), "entry far past the records": dict(brick_of=_set(3, 1 << 30)),
        "entry -2": dict(brick_of=_set(0, -2)),
        "repeated slot": dict(brick_of=_set(4, 3)), "slots out of order": dict(brick_of=_swap(2, 5)),
        "resolution of two": dict(resolution=np.asarray(RES[:2], dtype=np.int32)), "hi below lo": dict(hi=np.asarray(LO, dtype=np.float64)),
        "negative threshold": dict(sigma_threshold=np.float64(-1.0)),
    }

    def forbidden(*a, **k):
        raise AssertionError("a damaged file reached the upload")
    for what, change in damage.items():
        path = str(tmp_path / "damaged.npz")
        _file(path, 8, **change)
        with pytest.raises(ValueError):
            baked.read_brick_file(path)
        with monkeypatch.context() as m:
            m.setattr(torch, "as_tensor", forbidden)
            with pytest.raises(ValueError):
                BrickBakedField.load(path, device="cpu")
    # a format-1 file, written by BakedField.save itself (host tensors: nothing here needs a device)
    dense = BakedField(torch.zeros((27, 32), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), (3, 3, 3), (LO, HI), 1)
    one = str(tmp_path / "dense.npz")
    dense.save(one)
    with pytest.raises(ValueError):
        baked.read_brick_file(one)
    # and BakedField.load keeps refusing a format-2 file
    two = str(tmp_path / "two.npz")
    _file(two, 8)
    with pytest.raises(ValueError, match="format"):
        BakedField.load(two, device="cpu")
    # the dispatcher refuses what is neither
    three = str(tmp_path / "three.npz")
    _file(three, 8, format=np.int32(3))
    with pytest.raises(ValueError, match="format"):
        baked.load_field(three)
    np.savez(str(tmp_path / "none.npz"), records=np.zeros(3))
    with pytest.raises(ValueError):
        baked.load_field(str(tmp_path / "none.npz"))


def test_save_writes_what_the_reader_reads(tmp_path):
    """BrickBakedField.save on host tensors (no device needed) -> read_brick_file: the same arrays; load_field dispatches on the format"""
    import torch
    from keras_nerf_amd import baked
    from keras_nerf_amd.baked import BrickBakedField
    from keras_nerf_amd.runtime import pack_occupancy
    _, _, rec, occ, brick_of, n = scene(2, 4)
    bricks = B.bricks_from_dense(rec, brick_of, n, RES, 4)
    words = pack_occupancy(occ).view(np.int32)
    field =BrickBakedField(torch.as_tensor(bricks), torch.as_tensor(brick_of), torch.as_tensor(words), RES, (LO, HI), 2, 4, 0.5)
    assert field.brick == 4 and field.n_bricks == n and field.resolution == RES and field.bounds == (LO, HI) and field.sh_degree == 2
    assert field.sigma_threshold == 0.5 and field.nbytes == bricks.nbytes + brick_of.nbytes + words.nbytes
    assert field.brick_of.dtype == torch.int32 and tuple(field.brick_of.shape) == brick_of.shape
    assert np.array_equal(field.occupied.numpy(), occ) and len(field.cell_size) == 3 and field.device.type == "cpu"
    assert not hasattr(field, "optimizer") and not hasattr(field, "resample")
    path = str(tmp_path / "scene")
    field.save(path)
    got = baked.read_brick_file(path)
    assert np.array_equal(got["records"], bricks) and np.array_equal(got["brick_of"], brick_of) and np.array_equal(got["words"], words)
    assert got["brick"] == 4 and got["sigma_threshold"] == 0.5 and got["resolution"] == RES and got["n_bricks"] == n
    again = baked.load_field(path, device="cpu")
    assert isinstance(again, BrickBakedField) and torch.equal(again._records, field._records) and again.brick == 4
    # to_dense on host tensors is the reference's dense table
    assert np.array_equal(field.to_dense()._records.numpy(), B.dense_from_bricks(bricks, brick_of, RES, 4))


@pytest.mark.parametrize("b", BRICKS)
def test_compact_and_to_dense_on_host_tensors(b):
    """the torch index plumbing of compact / to_dense runs on host tensors too: against the reference, byte for byte"""
    import torch
    from keras_nerf_amd.baked import BakedField
    from keras_nerf_amd.runtime import pack_occupancy
    _, _, rec, occ, brick_of, n = scene(3, b)
    words = torch.as_tensor(pack_occupancy(occ).view(np.int32))
    dense = BakedField(torch.as_tensor(rec), words, RES, (LO, HI), 3, 0.25)
    field = dense.compact(b)
    assert field.brick == b and field.n_bricks == n and field.sigma_threshold == 0.25 and field._words is words
    assert np.array_equal(field.brick_of.numpy(), brick_of) and field.brick_of.dtype == torch.int32
    want = B.bricks_from_dense(rec, brick_of, n, RES, b)
    assert np.array_equal(field._records.numpy(), want)
    assert np.array_equal(field.to_dense()._records.numpy(), B.dense_from_bricks(want, brick_of, RES, b))
    assert np.array_equal(dense._records.numpy(), rec)                     # the dense field is left as it is
    # no occupied cell: one zero brick that no entry names
    none = BakedField(torch.as_tensor(rec), torch.zeros_like(words), RES, (LO, HI), 3).compact(b)
    assert none.n_bricks == 1 and not none._records.any() and (none.brick_of == -1).all() and not none.to_dense()._records.any()


def test_python_surface_refuses_bad_arguments():
    import torch
    from keras_nerf_amd import baked
    from keras_nerf_amd.baked import BakedField, BrickBakedField
    assert baked.check_brick(4) == 4 and baked.check_brick(np.int64(8)) == 8 and baked.DEFAULT_BRICK in baked.BRICKS
    for bad in (0, 2, 5, 16, 8.0, True, "8", None, (8,)):
        with pytest.raises(ValueError, match="brick"):
            baked.check_brick(bad)
        with pytest.raises(ValueError, match="brick"):
            baked.brick_table(np.zeros((2, 2, 2), dtype=bool), (3, 3, 3), bad)
    with pytest.raises(ValueError, match="occupied"):
        baked.brick_table(np.zeros((3, 3, 3), dtype=bool), (3, 3, 3), 8)
    dense = BakedField(torch.zeros((27, 16), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), (3, 3, 3), (LO, HI), 0)
    for bad in (5, 16, None, 8.0):
        with pytest.raises(ValueError, match="brick"):
            dense.compact(bad)
    rec, table, words = torch.zeros((1, 512, 16), dtype=torch.uint8), torch.full((1, 1, 1), -1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    for args in ((rec, table, words, (3, 3, 3), (LO, HI), 0, 5), (rec, table, words, (3, 3, 3), (LO, HI), 4, 8),
                 (rec, table, words, (3, 3, 3), (LO, HI), 1, 8), (rec, table, words, (3, 3, 3), (LO, HI), 0, 4),
                 (rec[:0], table, words, (3, 3, 3), (LO, HI), 0, 8), (rec, table, words, (9, 3, 3), (LO, HI), 0, 8),
                 (rec.reshape(512, 16), table, words, (3, 3, 3), (LO, HI), 0, 8)):
        with pytest.raises(ValueError):
            BrickBakedField(*args)
    # render: refused on the host, before the library is asked (the tensors here are not even on a device)
    field = BrickBakedField(rec, table, words, (3, 3, 3), (LO, HI), 0, 8)
    o, d = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    for bad in (dict(step=-1.0), dict(step=0.0), dict(step=float("nan")), dict(termination=1.0), dict(termination=-0.1),
                dict(outputs=("rgb",)), dict(outputs=()), dict(outputs=("image", "image")), dict(lanes_per_ray=2), dict(lanes_per_ray=4)):
        with pytest.raises(ValueError):
            field.render(o, d, 0.0, 6.0, **bad)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID decided on the host: no device is needed and no pointer is dereferenced"""
    import ctypes as C
    from keras_nerf_amd import _lib
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    p = C.c_void_p(4096)

    def render(res=(19, 17, 12), degree=2, lo=LO, hi=HI, records=p, brick_of=p, bits=p, log2=3, n_bricks=11, null=False, o=p, d=p,
               near=None, far=None, near_all=2.0, far_all=6.0, n_rays=0, step=0.02, eps=0.0, flags=_lib.BAKED_SKIP_EMPTY, image=p,
               depth=None, opacity=None, stats=None):
        f = _lib.KnerfBakedBricks(records, brick_of, bits, (C.c_int32 * 3)(*res), degree, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), log2,
                                  n_bricks)
        return lib.knerf_baked_render_bricks(None, None if null else C.byref(f), o, d, near, far, near_all, far_all, n_rays, step, eps,
                                             flags, image, depth, opacity, stats)

    lanes = lambda n: _lib.BAKED_SKIP_EMPTY | (n << _lib.BAKED_LANES_SHIFT)
    # good arguments and no ray: KNERF_OK without a launch, for both brick sizes, every table size the lattice admits and no bits
    assert render() == 0 and render(log2=2, n_bricks=75) == 0 and render(n_bricks=18) == 0 and render(n_bricks=1) == 0
    assert render(bits=None, flags=0) == 0 and render(flags=lanes(4)) == 0 and render(degree=1, flags=lanes(2)) == 0
    nan, inf = float("nan"), float("inf")
    for bad in (
            # what knerf_baked_render refuses
            dict(null=True), dict(records=None), dict(o=None), dict(d=None), dict(image=None), dict(degree=-1), dict(degree=4),
            dict(res=(1, 17, 12)), dict(res=(19, 1026, 12)), dict(res=(19, 17, 0)), dict(hi=(1.0, -0.8, 0.7)), dict(lo=(nan, -0.8, -0.6)),
            dict(hi=(inf, 0.8, 0.7)), dict(step=0.0), dict(step=-0.02), dict(step=nan), dict(step=inf), dict(eps=1.0), dict(eps=-0.1),
            dict(eps=nan), dict(flags=4), dict(flags=1 << 12), dict(flags=lanes(2)), dict(flags=lanes(3)), dict(degree=1, flags=lanes(4)),
            dict(degree=0, flags=lanes(2)), dict(bits=None), dict(n_rays=1 << 36), dict(near_all=nan), dict(far_all=inf),
            # and what the brick table adds
            dict(brick_of=None), dict(log2=0), dict(log2=1), dict(log2=4), dict(log2=-3), dict(n_bricks=0), dict(n_bricks=19),
            dict(log2=2, n_bricks=76), dict(n_bricks=1 << 40), dict(n_bricks=(1 << 64) - 1),
            dict(res=(1025, 1025, 1025), degree=3, log2=2, n_bricks=(1 << 40) // (64 * 112) + 1)):
        assert render(**bad) == INV, bad
    # the last one above is refused as "more bricks than the grid has" as well: no lattice of at most 1025 points per axis has
    # enough bricks for 2^40 bytes, so the size bound of the ABI can only be met together with the count bound
    assert 257 ** 3 * 64 * 112 < 1 << 40 and 129 ** 3 * 512 * 112 < 1 << 40
