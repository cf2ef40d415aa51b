"""Optimising a brick baked field, the parts that need no GPU: the package's train-brick set, flags and master rows
(keras_nerf_amd/baked_bricks_train.py train_state) and the gather behind finish() (kept_bricks) on host tensors against
tests/baked_bricks_train_reference.py, the argument checks of the Python surface and of both entry points, and that the helpers of
the march are defined once (csrc/baked_common.h).  Every condition is stated in tests/README_baked_bricks_train.md."""
import numpy as np
import pytest

from tests import baked_bricks_reference as B
from tests import baked_bricks_train_reference as S
from tests import baked_reference as R
from tests import baked_train_reference as T
from tests.test_baked_bricks_host import BRICKS, HI, LO, RES
from tests.test_baked_bricks_host import lattice as two_blobs


def lattice(degree, seed=0, shrink=1.0):
    """the two blobs of tests/test_baked_bricks_host.py and a third, the single point (14, 2, 2).  The touched points of the two blobs
    stay inside their bricks when the support grows by a cell, for both brick sizes; the third's reach x = 13..15, and 12..16 after
    one dilation: brick x = 2 (b = 8) resp. 4 (b = 4) is then new.  shrink scales the coefficients above order 0 (the GPU tests
    against fp64 use it to keep colours off the clamp edges)."""
    sigma, co = two_blobs(degree, seed)
    sigma[14, 2, 2] = np.float32(7.0)
    if shrink != 1.0:
        co[..., 1:, :] = (co[..., 1:, :].astype(np.float32) * np.float32(shrink)).astype(np.float16)
    return sigma, co


def scene(degree, b):
    """(sigma, coefficients, dense records, occupied cells, brick_of, n_bricks, brick records) of the lattice above, from the NumPy
    references"""
    from tests import baked_grow_reference as G
    sigma, co = lattice(degree)
    occ = R.occupied_cells(sigma)
    brick_of, n = B.brick_table(occ, RES, b)
    rec = G.pack(sigma, co, degree)
    return sigma, co, rec, occ, brick_of, n, B.bricks_from_dense(rec, brick_of, n, RES, b)


def words_of(cells):
    import torch
    from keras_nerf_amd.runtime import pack_occupancy
    return torch.as_tensor(pack_occupancy(cells).view(np.int32))


def source(degree, b):
    """the brick field of the scene on host tensors"""
    import torch
    from keras_nerf_amd.baked import BrickBakedField
    _, _, _, occ, brick_of, _, bricks = scene(degree, b)
    return BrickBakedField(torch.as_tensor(bricks), torch.as_tensor(brick_of), words_of(occ), RES, (LO, HI), degree, b, 0.0)


@pytest.mark.parametrize("b", BRICKS)
def test_the_lattice_has_what_the_tests_need(b):
    sigma, co, _, occ, brick_of, n, _ = scene(2, b)
    same, of0, n0 = S.train_bricks(sigma, b, 0)
    grown, of1, n1 = S.train_bricks(sigma, b, 1)
    assert np.array_equal(same, occ) and np.array_equal(of0, brick_of) and n0 == n                 # dilation 0: the field's own bricks
    assert ((of1 >= 0) & (brick_of < 0)).sum() >= 1 and ((of1 >= 0) | (brick_of < 0)).all() and n1 > n   # dilation 1: more of them
    assert (of1 < 0).any() and B.partial_edge_bricks(of1, RES, b).any()
    flags = S.flags(grown, of1, b)
    slot, train = (flags & 1) != 0, (flags & 2) != 0
    assert slot.sum() == T.slot_points(grown).sum() and train.sum() == T.sigma_trainable(grown).sum()
    assert 0 < train.sum() < slot.sum() < flags.size and not (train & ~slot).any()
    # rows per slot: the price of one row per stored record
    assert flags.size / slot.sum() > 1.1
    # the dense arrays of the brick field: absent bricks lose their coefficients, nothing else changes
    sg, cf = S.dense_arrays(scene(2, b)[6], brick_of, RES, b, 2)
    assert np.array_equal(sg, sigma) and (cf != co).any()
    x, y, z = np.meshgrid(*(np.arange(r) for r in RES), indexing="ij")
    stored = brick_of[x // b, y // b, z // b] >= 0
    assert np.array_equal(cf[stored].view(np.uint16), co[stored].view(np.uint16)) and not cf[~stored].any()


@pytest.mark.parametrize("dilation", [0, 1])
@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("degree", [0, 2])
def test_train_state_equals_the_reference(degree, b, dilation):
    from keras_nerf_amd.baked_bricks_train import train_state
    sigma, _, _, _, brick_of, _, bricks = scene(degree, b)
    field = source(degree, b)
    support, want_of, n = S.train_bricks(sigma, b, dilation)
    got_of, records, flags, master = train_state(field, words_of(support))
    assert got_of.numpy().dtype == np.int32 and np.array_equal(got_of.numpy(), want_of) and records.shape[0] == n
    sg, cf = S.dense_arrays(bricks, brick_of, RES, b, degree)
    from tests import baked_grow_reference as G
    want = B.bricks_from_dense(G.pack(sg, cf, degree), want_of, n, RES, b)
    assert np.array_equal(records.numpy(), want)
    assert flags.numpy().dtype == np.uint8 and np.array_equal(flags.numpy(), S.flags(support, want_of, b))
    rows = master.numpy()
    assert rows.dtype == np.float32 and np.array_equal(rows, S.master_rows(sg, cf, support, want_of, b))
    # the source is left as it is, and the added bricks start as zero records
    assert np.array_equal(field._records.numpy(), bricks)
    added = want_of[(want_of >= 0) & (brick_of < 0)]
    assert (len(added) > 0) == (dilation == 1) and not records.numpy()[added].any()


@pytest.mark.parametrize("b", BRICKS)
def test_brick_sigma_on_host_tensors(b):
    from keras_nerf_amd.baked_bricks_train import brick_sigma
    sigma, _, _, _, brick_of, n, bricks = scene(1, b)
    stored, dense = brick_sigma(source(1, b))
    assert np.array_equal(dense.numpy(), sigma)
    assert np.array_equal(stored.numpy(), np.ascontiguousarray(bricks[:, :, :4]).view(np.float32).reshape(-1))
    cut_stored, cut = brick_sigma(source(1, b), 10.0)
    want = np.where(sigma > 10.0, sigma, 0).astype(np.float32)
    assert np.array_equal(cut.numpy(), want) and (want != sigma).any() and cut_stored.numpy().max() == want.max()


@pytest.mark.parametrize("b", BRICKS)
def test_kept_bricks_is_the_dense_finish_then_compact(b):
    """the gather behind finish() on host tensors: the live field of a dilated optimiser, sigma cut at a threshold that empties the
    third blob, against thresholding the dense records and cutting them into bricks"""
    import torch
    from keras_nerf_amd.baked import BrickBakedField
    from keras_nerf_amd.baked_bricks_train import brick_sigma, kept_bricks, train_state
    from tests import baked_grow_reference as G
    degree, thr = 2, 7.5
    sigma, _, _, _, brick_of, n, bricks = scene(degree, b)
    field = source(degree, b)
    support, train_of, _ = S.train_bricks(sigma, b, 1)
    got_of, records, _, _ = train_state(field, words_of(support))
    live = BrickBakedField(records, got_of, words_of(support), RES, (LO, HI), degree, b, 0.0)
    stored, dense = brick_sigma(live, thr)
    cut = np.where(sigma > thr, sigma, 0).astype(np.float32)
    assert np.array_equal(dense.numpy(), cut) and cut[14, 2, 2] == 0 and cut.any()
    occ = R.occupied_cells(cut)
    done = kept_bricks(live, stored, words_of(occ), thr)
    want_of, want_n = B.brick_table(occ, RES, b)
    assert type(done) is BrickBakedField and done.sigma_threshold == thr and done.brick == b
    assert np.array_equal(done.brick_of.numpy(), want_of) and done.n_bricks == want_n < records.shape[0]
    _, cf = S.dense_arrays(bricks, brick_of, RES, b, degree)
    assert np.array_equal(done._records.numpy(), B.bricks_from_dense(G.pack(cut, cf, degree), want_of, want_n, RES, b))
    # nothing is left: one all-zero brick that no entry names, as BakedField.compact gives
    none = kept_bricks(live, torch.zeros_like(stored), words_of(np.zeros_like(occ)), thr)
    assert none.n_bricks == 1 and not none._records.any() and (none.brick_of == -1).all()


def test_the_optimiser_is_reached_through_baked_train_and_not_through_the_field():
    from keras_nerf_amd import baked, baked_bricks_train, baked_train
    from keras_nerf_amd.baked import BrickBakedField
    assert baked_train.BrickFieldOptimizer is baked_bricks_train.BrickFieldOptimizer is baked.BrickFieldOptimizer
    assert baked.brick_optimizer is baked_train.brick_optimizer
    assert baked_train.BRICK_TRAIN_VARIANTS == {0: (1,), 1: (1, 2), 2: (1, 4), 3: (1, 4)}
    with pytest.raises(AttributeError):
        baked_train.no_such_name
    field = source(0, 8)
    assert not hasattr(field, "optimizer") and not hasattr(BrickBakedField, "optimizer") and not hasattr(field, "resample")
    for name in ("accumulate", "apply", "train_step", "fit", "gradients", "slot_mask", "sigma_trainable", "finish", "nbytes"):
        assert hasattr(baked_train.BrickFieldOptimizer, name), name
    for name in ("regularize", "tv_weights", "regularized"):
        assert not hasattr(baked_train.BrickFieldOptimizer, name), name


def test_python_surface_refuses_bad_arguments(monkeypatch):
    """every refusal comes before the first launch: the fields here live on the host and the occupancy launch is forbidden"""
    import torch
    from keras_nerf_amd import baked_train, runtime
    from keras_nerf_amd.baked import BakedField
    from keras_nerf_amd.baked_bricks_train import check_brick_lanes

    def forbidden(*a, **k):
        raise AssertionError("a refused argument reached a launch")
    monkeypatch.setattr(runtime, "occupancy_words_from_grid", forbidden)
    good = dict(learning_rate_sigma=0.05, learning_rate_sh=0.01)
    field = source(2, 8)
    for kw in (dict(learning_rate_sigma=0.0), dict(learning_rate_sh=-1.0), dict(learning_rate_sh=float("nan")), dict(beta_1=1.0),
               dict(beta_2=-0.5), dict(epsilon=0.0), dict(dilation=-1), dict(dilation=9), dict(dilation=1.5), dict(termination=1.0),
               dict(termination=-0.1), dict(step=0.0), dict(step=float("inf")), dict(lanes_per_ray=2), dict(lanes_per_ray=3),
               dict(lanes_per_ray=8), dict(lanes_per_ray=True), dict(lanes_per_ray=4.0)):
        with pytest.raises(ValueError):
            baked_train.brick_optimizer(field, **{**good, **kw})
    for degree, lanes in ((0, 2), (0, 4), (1, 4), (3, 2)):
        with pytest.raises(ValueError, match="lanes_per_ray"):
            baked_train.brick_optimizer(source(degree, 4), lanes_per_ray=lanes, **good)
    for degree, lanes in baked_train.BRICK_TRAIN_VARIANTS.items():
        assert [check_brick_lanes(degree, n) for n in (0,) + lanes] == [0, *lanes]
    # the total-variation regulariser belongs to the dense optimiser
    for kw in (dict(tv_sigma=0.1), dict(tv_sh=0.1), dict(tv_epsilon=1e-6)):
        with pytest.raises(TypeError):
            baked_train.brick_optimizer(field, **good, **kw)
        with pytest.raises(TypeError):
            baked_train.BrickFieldOptimizer(field, **good, **kw)
    dense = BakedField(torch.zeros((27, 16), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), (3, 3, 3), (LO, HI), 0)
    with pytest.raises(ValueError, match="BrickBakedField"):
        baked_train.brick_optimizer(dense, **good)
    # with good arguments the construction gets as far as the support's launch
    with pytest.raises(AssertionError, match="reached a launch"):
        baked_train.brick_optimizer(field, **good)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID decided on the host: no device is needed and no pointer is dereferenced"""
    import ctypes as C
    from keras_nerf_amd import _lib
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    p = C.c_void_p(4096)                                                  # never dereferenced: every call below is refused first

    def state(res=(19, 17, 12), degree=2, lo=LO, hi=HI, records=p, brick_of=p, bits=p, log2=3, n_bricks=11, grad=p):
        f = _lib.KnerfBakedBricks(records, brick_of, bits, (C.c_int32 * 3)(*res), degree, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), log2,
                                  n_bricks)
        return _lib.KnerfBakedBricksTrain(f, grad)

    def rays(st, o=p, d=p, target=p, n=0, n_norm=0, step=0.02, term=0.0, flags=0, near_all=0.0, far_all=1.0):
        return lib.knerf_baked_bricks_train_rays(None, C.byref(st) if st is not None else None, o, d, None, None, near_all, far_all,
                                                 target, n, n_norm, step, term, flags, None)

    def apply(st, flags=p, w=p, m=p, v=p, rs=0.1, rc=0.01, b1=0.9, b2=0.999, eps=1e-7):
        return lib.knerf_baked_bricks_train_apply(None, C.byref(st) if st is not None else None, flags, w, m, v, rs, rc, b1, b2, eps)

    lanes = lambda n: n << _lib.BAKED_LANES_SHIFT
    # good arguments and no ray: KNERF_OK without a launch, for both brick sizes and every lane variant that exists
    assert rays(state()) == 0 and rays(state(log2=2, n_bricks=75)) == 0 and rays(state(n_bricks=18)) == 0 and rays(state(n_bricks=1)) == 0
    from keras_nerf_amd.baked_train import BRICK_TRAIN_VARIANTS
    for degree in range(4):
        for n in (1, 2, 4):
            want = 0 if n in BRICK_TRAIN_VARIANTS[degree] else INV
            assert rays(state(degree=degree), flags=lanes(n)) == want, (degree, n)
            if want == INV:                                               # refused with rays too: nothing is launched
                assert rays(state(degree=degree), flags=lanes(n), n=10) == INV
    nan, inf = float("nan"), float("inf")
    for call in (rays, apply):
        assert call(None) == INV
        for bad in (
                # what knerf_baked_render_bricks refuses of its field
                dict(records=None), dict(brick_of=None), dict(degree=-1), dict(degree=4), dict(res=(1, 17, 12)), dict(res=(19, 1026, 12)),
                dict(res=(19, 17, 0)), dict(hi=(1.0, -0.8, 0.7)), dict(lo=(nan, -0.8, -0.6)), dict(hi=(inf, 0.8, 0.7)), dict(log2=0),
                dict(log2=1), dict(log2=4), dict(log2=-3), dict(n_bricks=0), dict(n_bricks=19), dict(log2=2, n_bricks=76),
                dict(n_bricks=1 << 40), dict(n_bricks=(1 << 64) - 1),
                dict(res=(1025, 1025, 1025), degree=3, log2=2, n_bricks=(1 << 40) // (64 * 112) + 1),
                # and what the optimiser adds
                dict(bits=None), dict(grad=None)):
            assert call(state(**bad)) == INV, (call.__name__, bad)
    for bad in (dict(o=None), dict(d=None), dict(target=None), dict(step=0.0), dict(step=-0.02), dict(step=nan), dict(step=inf),
                dict(term=1.0), dict(term=-0.1), dict(term=nan), dict(flags=4), dict(flags=1 << 12), dict(flags=lanes(2)), dict(flags=lanes(3)),
                dict(n=1 << 36), dict(n_norm=1 << 36), dict(near_all=nan), dict(far_all=inf)):
        assert rays(state(), **bad) == INV, bad
    for bad in (dict(flags=None), dict(w=None), dict(m=None), dict(v=None), dict(rs=nan), dict(rc=inf), dict(b1=1.0), dict(b2=-0.1),
                dict(eps=0.0), dict(eps=nan)):
        assert apply(state(), **bad) == INV, bad


def test_the_march_helpers_and_the_adam_column_are_defined_once_in_the_shared_header():
    """the dense and the brick optimiser run ONE march (csrc/baked_train.hip), and what they share with the other baked*.hip files --
    sh_eval, the DPP group sums, locate, the Adam column, the record's sizes and codec -- is defined once, in csrc/baked_common.h"""
    import os
    from keras_nerf_amd import baked
    from tests.test_baked_train_host import MARCH_HELPERS, defined_once_in_the_header
    defined_once_in_the_header(MARCH_HELPERS + ("__device__ __forceinline__ float adam(",))
    src = open(os.path.join(os.path.dirname(os.path.abspath(baked.__file__)), "csrc", "baked_train.hip")).read()
    assert src.count("__device__ __forceinline__ void march(") == 1 and src.count("void baked_train_rays_kernel(") == 1
    assert "knerf_baked_train_rays(" in src and "knerf_baked_bricks_train_rays(" in src
