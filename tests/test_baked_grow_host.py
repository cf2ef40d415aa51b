"""Growing a baked field, the parts that need no GPU: the NumPy reference's TV gradient (tests/baked_grow_reference.py) against central
differences of its own fp64 value, the float32 resampling mirror against float64, the exact properties of resampling, and the
host-side argument checks of keras_nerf_amd/baked.py, baked_train.py and of the two entry points.  Tolerances are derived in
tests/README_baked_grow.md; the measured values stand there too."""
import numpy as np
import pytest

from tests import baked_grow_reference as G

RES = (4, 4, 3)
EPS = 1e-2
H = 1e-5
W_SIGMA, W_SH = 0.7, 0.3


def _slots():
    """4 x 4 x 3 with two support holes: every point but (1, 1, 1) and (3, 2, 0) has a slot"""
    has = np.ones(RES, dtype=bool)
    has[1, 1, 1] = has[3, 2, 0] = False
    slot_of = np.full(has.size, -1, dtype=np.int64)
    slot_of[has.reshape(-1)] = np.arange(int(has.sum()))
    return has, slot_of


@pytest.mark.parametrize("degree", [0, 2])
def test_tv_gradient_matches_central_differences(degree):
    has, slot_of = _slots()
    n, W = int(has.sum()), 1 + 3 * (degree + 1) ** 2
    rng = np.random.default_rng(7 + degree)
    master = rng.normal(0.0, 0.5, (n, W))
    master[:, 0] = np.abs(master[:, 0]) * 4.0
    master[5:9] = master[5]                                                # equal neighbours along z: D = 0 there
    R, grad, sums = G.tv_value_and_grad(master, slot_of, RES, W_SIGMA, W_SH, EPS)
    assert R == pytest.approx(W_SIGMA * sums[0] + W_SH * sums[1], rel=1e-15) and sums[0] > 0 and sums[1] > 0

    def value(m):
        return G.tv_value_and_grad(m, slot_of, RES, W_SIGMA, W_SH, EPS)[0]
    entries = [(s, 0) for s in range(n)]                                   # every sigma
    if W > 1:
        flat = rng.choice(n * (W - 1), 40, replace=False)                  # and forty coefficient entries drawn at random
        entries += [(int(e // (W - 1)), 1 + int(e % (W - 1))) for e in flat]
    worst = 0.0
    for s, q in entries:
        a, b = master.copy(), master.copy()
        a[s, q] += H; b[s, q] -= H
        worst = max(worst, abs((value(a) - value(b)) / (2 * H) - grad[s, q]))
    # truncation h^2 / 6 |R'''| with |R'''| <= 7.04 w / eps per variable, rounding 8 x 2^-53 |R| / h (README_baked_grow.md)
    tol = H * H / 6.0 * 7.04 * max(W_SIGMA, W_SH) / EPS + 8.0 * 2.0 ** -53 * abs(R) / H
    print(f"degree {degree}: max |fd - analytic| = {worst:.3e} (tolerance {tol:.3e}, max |g| {np.abs(grad).max():.3e}, R {R:.4e})")
    assert np.abs(grad).max() > 0.3 and worst <= tol
    # the float32 form is the same function
    R32, grad32, _ = G.tv_value_and_grad(master.astype(np.float32), slot_of, RES, W_SIGMA, W_SH, EPS, dtype=np.float32)
    assert grad32.dtype == np.float32 and abs(R32 - R) < 1e-5 * R and np.abs(grad32 - grad).max() < 1e-4


def test_tv_ignores_points_without_a_slot_and_zero_weights():
    has, slot_of = _slots()
    n = int(has.sum())
    rng = np.random.default_rng(3)
    master = rng.normal(0.0, 1.0, (n, 4))
    R, grad, sums = G.tv_value_and_grad(master, slot_of, RES, 1.0, 0.0, EPS)
    assert (grad[:, 1:] == 0).all() and np.abs(grad[:, 0]).max() > 0 and R == pytest.approx(sums[0])
    # a constant field has D = 0 everywhere: every term is sqrt(eps) and the gradient vanishes
    R, grad, sums = G.tv_value_and_grad(np.ones((n, 4)), slot_of, RES, 1.0, 1.0, EPS)
    assert (grad == 0).all() and sums[0] == pytest.approx(n * np.sqrt(EPS)) and sums[1] == pytest.approx(3 * n * np.sqrt(EPS))
    # a lone slot: no neighbour, no difference
    lone = np.full(has.size, -1, dtype=np.int64); lone[17] = 0
    R, grad, _ = G.tv_value_and_grad(np.array([[3.0, 1.0, 2.0, 5.0]]), lone, RES, 1.0, 1.0, EPS)
    assert (grad == 0).all() and R == pytest.approx(4 * np.sqrt(EPS))


def _table(res, degree, seed=0):
    rng = np.random.default_rng(60 + seed)
    K = (degree + 1) ** 2
    sigma = rng.uniform(0.0, 30.0, res).astype(np.float32)
    sigma[2:4, 1:3, 1:3] = 0                                               # one old cell with sigma = 0 at its 8 corners
    sigma[-2:] = 0                                                         # and a layer of such cells
    co = (rng.standard_normal(res + (K, 3)) * 0.5).astype(np.float16)
    return sigma, co, G.pack(sigma, co, degree)


@pytest.mark.parametrize("res_new", [(17, 13, 11), (12, 9, 8), (5, 4, 3), (2, 2, 2), (23, 7, 40)])
def test_float32_resampling_mirror_against_float64(res_new):
    res, degree = (9, 7, 6), 2
    sigma, co, rec = _table(res, degree)
    s32, c32, r32 = G.resample(rec, res, res_new, degree, 0.0, np.float32)
    s64, c64, none = G.resample(rec, res, res_new, degree, 0.0, np.float64)
    assert none is None and s32.dtype == np.float32 and c32.dtype == np.float32 and r32.shape == (int(np.prod(res_new)), 64)
    bound_s = 16 * 2.0 ** -24 * G.corner_max(sigma, res, res_new)
    bound_c = 16 * 2.0 ** -24 * G.corner_max(co, res, res_new)
    err_s, err_c = np.abs(s32 - s64), np.abs(c32 - c64)
    rel = max(float((err_s / np.maximum(bound_s, 1e-300)).max()), float((err_c / np.maximum(bound_c, 1e-300)).max()))
    print(f"{res} -> {res_new}: largest error / bound = {rel:.3f}")
    assert (err_s <= bound_s).all() and (err_c <= bound_c).all()


def test_exact_properties_of_resampling():
    res, degree = (9, 7, 6), 2
    sigma, co, rec = _table(res, degree)
    K = 9
    # R' = 2 R - 1: every old point reappears with its values unchanged as numbers
    fine = (17, 13, 11)
    s, _, r = G.resample(rec, res, fine, degree)
    sg, cf = G.unpack(r, degree)
    sg, cf = sg.reshape(fine), cf.reshape(fine + (K, 3))
    assert np.array_equal(sg[::2, ::2, ::2], sigma) and np.array_equal(cf[::2, ::2, ::2].astype(np.float32), co.astype(np.float32))
    assert np.array_equal(s, sg)
    # the first and last point of each axis are kept for any R'
    for res_new in ((12, 9, 8), (5, 4, 3), (2, 2, 2), (31, 5, 17)):
        sg, cf = G.unpack(G.resample(rec, res, res_new, degree)[2], degree)
        sg, cf = sg.reshape(res_new), cf.reshape(res_new + (K, 3))
        ends = np.ix_((0, -1), (0, -1), (0, -1))
        assert np.array_equal(sg[ends], sigma[ends]) and np.array_equal(cf[ends].astype(np.float32), co[ends].astype(np.float32))
    # an old cell with sigma = 0 at its 8 corners: sigma = 0 at every new point inside it
    for res_new in (fine, (12, 9, 8), (40, 30, 20)):
        sg = G.resample(rec, res, res_new, degree)[0]
        cells = [G.placement(r, rn)[0] for r, rn in zip(res, res_new)]
        cx, cy, cz = np.meshgrid(*cells, indexing="ij")
        empty = np.zeros(tuple(r - 1 for r in res), dtype=bool)
        empty[2, 1, 1] = True; empty[7:] = True
        inside = empty[cx, cy, cz]
        assert inside.sum() > 0 and (sg[inside] == 0).all() and (sg >= 0).all()
    # the threshold: what is <= it is exactly 0, what is above it is untouched
    plain = G.resample(rec, res, (12, 9, 8), degree, 0.0)[0]
    cut = G.resample(rec, res, (12, 9, 8), degree, 10.0)[0]
    assert ((cut == 0) | (cut > 10.0)).all() and np.array_equal(cut[plain > 10.0], plain[plain > 10.0]) and (cut == 0).sum() > (plain == 0).sum()
    # the padding is zero
    for deg in (0, 1, 2, 3):
        _, _, rc = _table((3, 3, 3), deg)
        out = G.resample(rc, (3, 3, 3), (4, 5, 3), deg)[2]
        used = 4 + 6 * (deg + 1) ** 2
        assert out.shape[1] == G.record_bytes(deg) and (out[:, used:] == 0).all()
    # (2, 2, 2) -> anything: one cell, the corners kept
    _, _, rc = _table((2, 2, 2), 1, seed=3)
    assert np.array_equal(G.resample(rc, (2, 2, 2), (2, 2, 2), 1)[2][:, :28], rc[:, :28])


def test_reference_layout_is_the_package_layout():
    from keras_nerf_amd import baked
    sigma, co, rec = _table((3, 4, 2), 3)
    assert np.array_equal(rec, baked.pack_records(sigma, co)) and G.record_bytes(3) == baked.record_bytes(3)


def test_python_surface_refuses_bad_arguments():
    import torch
    from keras_nerf_amd import baked, baked_train
    from keras_nerf_amd.baked import BakedField, refined_resolution
    assert refined_resolution(128) == (255, 255, 255) and refined_resolution((9, 7, 6)) == (17, 13, 11) and refined_resolution(513) == (1025,) * 3
    for bad in (514, (9, 7, 600), 1, (9, 7), 9.0, True, "9", None):
        with pytest.raises(ValueError):
            refined_resolution(bad)
    # resample: refused on the host, before the library is asked (the tensors here are not even on a device)
    rec = torch.zeros((27, 16), dtype=torch.uint8)
    field = BakedField(rec, torch.zeros(1, dtype=torch.int32), (3, 3, 3), ((-1.0,) * 3, (1.0,) * 3), 0)
    for bad in (1, 1026, (3, 3), (3, 3, 1.5), None, "5"):
        with pytest.raises(ValueError, match="resolution"):
            field.resample(bad)
    for bad in (-1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="sigma_threshold"):
            field.resample(5, sigma_threshold=bad)
    good = dict(resolution=8, bounds=((-1.0,) * 3, (1.0,) * 3), sh_degree=1)
    for key, bad in (("resolution", 1), ("resolution", 2000), ("bounds", ((1.0,) * 3, (1.0,) * 3)), ("sh_degree", 4), ("sh_degree", 1.0),
                     ("sigma", -0.1), ("sigma", float("nan")), ("sigma", "1"), ("colour", float("inf")), ("colour", None), ("colour", 1e9)):
        with pytest.raises(ValueError):
            BakedField.uniform(**{**good, key: bad})
    assert baked.check_tv_args is baked_train.check_tv_args and baked.fit_coarse_to_fine is baked_train.fit_coarse_to_fine
    assert baked_train.check_tv_args(0, 1e-3, 1e-6) == (0.0, 1e-3, 1e-6)
    for key, bad in (("tv_sigma", -1e-3), ("tv_sigma", float("nan")), ("tv_sh", -1.0), ("tv_sh", float("inf")), ("tv_sh", "1"),
                     ("tv_epsilon", 0.0), ("tv_epsilon", -1e-6), ("tv_epsilon", 1e-60), ("tv_epsilon", True)):
        with pytest.raises(ValueError, match="tv_"):
            baked_train.check_tv_args(**{**dict(tv_sigma=0.0, tv_sh=0.0, tv_epsilon=1e-6), key: bad})
    assert baked_train.check_stages([(None, 3), ((5, 4, 3), 0)]) == [(None, 3), ((5, 4, 3), 0)]
    for bad in ([], None, [(None,)], [(None, -1)], [(None, 1.5)], [(None, True)], 5):
        with pytest.raises(ValueError, match="stage"):
            baked_train.check_stages(bad)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID decided on the host: no device is needed and no pointer is dereferenced"""
    import ctypes as C
    from keras_nerf_amd import _lib
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    p, far = C.c_void_p(4096), C.c_void_p(1 << 40)

    def field(res=(9, 7, 6), degree=2, lo=(-1.0,) * 3, hi=(1.0,) * 3, records=p, bits=p):
        return _lib.KnerfBakedField(records, bits, (C.c_int32 * 3)(*res), degree, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi))

    def tv(res=(9, 7, 6), degree=2, slot_of=p, grad=p, n_slots=10, point_of=p, master=p, ws=1e-3, wc=1e-3, eps=1e-6, out=None, null=False,
           **kw):
        st = _lib.KnerfBakedTrain(field(res, degree, **kw), slot_of, grad, n_slots)
        return lib.knerf_baked_train_tv(None, None if null else C.byref(st), point_of, master, ws, wc, eps, out)

    assert tv(ws=0.0, wc=0.0) == 0                                         # both weights 0 and no tv_out: nothing is launched
    for bad in (dict(null=True), dict(records=None), dict(bits=None), dict(slot_of=None), dict(grad=None), dict(point_of=None),
                dict(master=None), dict(degree=4), dict(degree=-1), dict(res=(1, 7, 6)), dict(res=(9, 1026, 6)),
                dict(hi=(1.0, -1.0, 1.0)), dict(lo=(float("nan"), -1.0, -1.0)), dict(n_slots=0), dict(n_slots=9 * 7 * 6 + 1),
                dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(ws=-1e-3), dict(wc=-1.0),
                dict(ws=float("nan")), dict(wc=float("inf"))):
        assert tv(**bad) == INV, bad

    def resample(new=(17, 13, 11), thr=0.0, dst=far, null=False, no_res=False, **kw):
        f = field(**kw)
        return lib.knerf_baked_resample(None, None if null else C.byref(f), None if no_res else (C.c_int32 * 3)(*new), thr, dst)

    for bad in (dict(null=True), dict(no_res=True), dict(dst=None), dict(records=None), dict(degree=4), dict(res=(1, 7, 6)),
                dict(res=(9, 7, 1026)), dict(new=(1, 13, 11)), dict(new=(17, 1026, 11)), dict(hi=(1.0, -1.0, 1.0)),
                dict(lo=(float("inf"), -1.0, -1.0)), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")),
                dict(dst=p), dict(dst=C.c_void_p(4096 + 64 * 100)), dict(dst=C.c_void_p(4096 - 64))):      # the last three: overlap
        assert resample(**bad) == INV, bad
