"""What tests/test_gpu_utils_ops.py rests on, without a device (tests/utils_ops_reference.py): the inputs hold the edges they promise,
the bounds computed from NumPy are not vacuous, and the two float32 mirrors of image_metrics_kernel's SSIM loop behave as measured.

SSIM mirrors against the float64 `oracle.ssim`, worst shape of `METRIC_SHAPES` per class (pytest -s prints every case):

| class | plain mirror (xx - mx mx on raw pixels) | pivoted mirror (moments about the window's centre pixel of A) |
|---|---|---|
| random +- 0.1 noise | 1.0e-7 | 1.8e-8 |
| A = 0.95, B = A + 1e-3 noise | **3.4e-4** | 1.1e-8 |
| A = 0.5, B = A + 1e-2 noise | 9.5e-6 | 1.7e-9 |
| both 0.95 + 1e-3 noise | **1.8e-4** | 4.0e-8 |
| white with a textured 10 x 10 patch | **5.2e-5** | 3.2e-9 |
| A = B | 0 | 0 |

The project's bound is atol 2e-5.  The plain form breaks it wherever a bright region is flat: xx and mx mx are both about 0.9 and agree in
their first four digits, so float32's 6e-8 relative rounding of each is an absolute 5e-8 beside c2 = 9e-4 plus a variance of 1e-6.
(The two textured classes: figures without the one-window 11 x 11 image, for which see
test_pivoted_mirror_meets_the_bound_with_a_margin_of_100.)"""
import numpy as np
import pytest

from oracle import nerf_oracle as O
from tests import utils_ops_reference as U

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def ssim_errors():
    out = {}
    for shape in U.METRIC_SHAPES:
        for kind in U.METRIC_CLASSES:
            a, b = U.metric_images(kind, shape)
            ref = O.ssim(a, b)
            out[shape, kind] = (float(np.abs(U.ssim_mirror(a, b, False) - ref).max()), float(np.abs(U.ssim_mirror(a, b, True) - ref).max()))
            print(f"{shape} {kind}: plain {out[shape, kind][0]:.2e}, pivoted {out[shape, kind][1]:.2e}, ssim {ref.min():.6f}")
    return out


def test_the_issue_s_own_case():
    """image A constant 0.95, B = A + 1e-3 N(0,1) clipped, (1, 32, 32, 3): the plain mirror is off by about 3e-4"""
    a, b = U.metric_images("flat_095_1e-3", (1, 32, 32, 3))
    ref = O.ssim(a, b)
    assert 0.998 < ref[0] < 0.9995
    assert 1e-4 < abs(U.ssim_mirror(a, b, False)[0] - ref[0]) < 1e-3
    assert abs(U.ssim_mirror(a, b, True)[0] - ref[0]) < 1e-8 * 2


def test_plain_mirror_breaks_the_bound_on_flat_bright_regions(ssim_errors):
    for shape in U.METRIC_SHAPES:
        for kind in ("flat_095_1e-3", "both_095_noise"):
            assert ssim_errors[shape, kind][0] > U.SSIM_ATOL, (shape, kind)
        assert ssim_errors[shape, "random"][0] < U.SSIM_ATOL / 10         # the existing test's kind of image hides it
    assert max(ssim_errors[s, "white_with_patch"][0] for s in U.METRIC_SHAPES) > U.SSIM_ATOL
    # A = 0.5 with 1e-2 noise: variance 1e-4 beside a cancellation error of 1.5e-8 -- the plain form is degraded (up to 9.5e-6,
    # half the bound) and the pivoted one is three orders better
    assert all(ssim_errors[s, "flat_05_1e-2"][0] > 100 * ssim_errors[s, "flat_05_1e-2"][1] for s in U.METRIC_SHAPES)


def test_pivoted_mirror_meets_the_bound_with_a_margin_of_100(ssim_errors):
    """on every flat class at every shape, and on the textured classes wherever an image has more than one window.  One single window
    of texture (the 11 x 11 image) has nothing to cancel and nothing to average: xx and mx mx are about 0.3 each, carry some
    sqrt(121) x 6e-8 x 0.3 = 2e-7 of accumulated rounding, and stand over sxx + syy + c2 of about 0.17, so either form is good to
    about 1e-6 there (measured: plain 6.0e-7 / 1.1e-7, pivoted 9.5e-7 / 3.5e-7): a margin of 10 is what is asserted for those two."""
    for (shape, kind), (_, pivoted) in ssim_errors.items():
        textured_single_window = shape == (1, 11, 11, 1) and kind in ("random", "white_with_patch")
        assert pivoted <= U.SSIM_ATOL / (10 if textured_single_window else 100), (shape, kind, pivoted)
    assert all(ssim_errors[s, "same"] == (0.0, 0.0) for s in U.METRIC_SHAPES)


def test_mirrors_agree_with_the_oracle_s_window():
    g = U.gauss11()
    assert g.dtype == f32 and abs(float(g.astype(f64).sum()) - 1) < 1e-6 and np.array_equal(g, g[::-1]) and g.argmax() == 5


def test_metric_classes_are_what_they_say():
    for shape in U.METRIC_SHAPES:
        for kind in U.METRIC_CLASSES:
            a, b = U.metric_images(kind, shape)
            assert a.shape == shape and b.shape == shape and a.dtype == f32 and b.dtype == f32
            assert a.min() >= 0 and a.max() <= 1 and b.min() >= 0 and b.max() <= 1
            assert np.array_equal(a, b) == (kind == "same")
        a, _ = U.metric_images("white_with_patch", shape)
        assert (a == 1).mean() > 0.05 and (a[:, :10, 1:11] < 1).mean() > 0.99
        a, _ = U.metric_images("flat_095_1e-3", shape)
        assert (a == f32(0.95)).all()


def test_posenc_inputs_and_bounds():
    for rows in U.POSENC_ROWS:
        x = U.posenc_inputs(rows)
        assert x.shape == (rows, 3) and x.dtype == f32
        assert np.signbit(x[x == 0]).any()                                     # a negative zero
        if rows > 1:
            nz = np.abs(x[x != 0])
            assert nz.min() <= 1e-3 and nz.max() >= 1e3 and (~np.signbit(x[x == 0])).any() and (x < 0).any() and (x > 0).any()
            for k in (1, 2, 3, 20):
                c = f32(k * np.pi / 2)
                assert {c, np.nextafter(c, f32(0)), np.nextafter(c, f32(100)), -c} <= set(x.reshape(-1).tolist())
        for L in U.POSENC_L:
            ref = U.posenc_float64(x, L)
            assert ref.shape == (rows, 3 + 6 * L) and np.array_equal(ref[:, :3], x.astype(f64))
            if L:
                # the argument is the exact product: a power of two times a float32
                assert np.array_equal(U.posenc_arguments(x, L).astype(f64), x.astype(f64)[:, None, :] * 2.0 ** np.arange(L)[None, :, None])
                assert np.array_equal(ref[:, 3:6], np.sin(x.astype(f64))) and np.array_equal(ref[:, 6:9], np.cos(x.astype(f64)))
            # NumPy's own float32 sin / cos stay within two float32 roundings of float64 on these arguments, 2^29 x 1e3 included
            assert U.POSENC_FLOOR <= U.posenc_bound(x, L) < 5e-7
    np.testing.assert_allclose(U.posenc_float64(U.posenc_inputs(85), 10), O.positional_encoding(U.posenc_inputs(85).astype(f64), 10), atol=1e-9)


def test_ray_points_reference_rounds_twice():
    rng = np.random.default_rng(0)
    o, d = rng.normal(0, 1, (257, 3)).astype(f32), rng.normal(0, 1, (257, 3)).astype(f32)
    t = rng.uniform(2, 6, (257, 7)).astype(f32)
    got = U.ray_points(o, d, t)
    fused = (o[:, None, :].astype(f64) + d[:, None, :].astype(f64) * t[:, :, None].astype(f64)).astype(f32)     # one rounding: an fma
    assert got.dtype == f32 and got.shape == (257, 7, 3) and (got != fused).any()
    assert np.abs(got - fused).max() <= 2 * np.spacing(f32(np.abs(d[:, None, :] * t[:, :, None]).max()))


def test_inverse_cdf_inputs_reach_both_out_of_range_modes():
    for nw, nm in U.INVERSE_CDF_SHAPES:
        mids, w, u = U.inverse_cdf_inputs(nw, nm, 5, 65)
        assert mids.shape == (5, nm) and w.shape == (5, nw) and u.shape == (5, 65) and u.min() == 0 and u.max() < 1
        z, c = (O.fine_hierarchical_sampling_chunk(mids, w, u, m) for m in ("zero", "clamp"))
        assert np.isfinite(z).all() and np.isfinite(c).all()
        assert np.array_equal(z, c) == (nm > nw)                               # with n_mid <= n_weights a gather goes past the end


def test_metrics_update_reference():
    st = np.zeros((6, 2))
    sc, sf = np.array([[90.0, 0.5], [80.0, 0.0]]), np.array([[95.0, 0.25], [85.0, 0.125]])
    st = U.metrics_update(st, sc, sf, None, (2, 11, 20, 1))
    assert st[:, 1].tolist() == [1, 2, 2, 1, 2, 2]
    assert st[1, 0] == np.inf and np.isfinite(st[[0, 2, 3, 4, 5], 0]).all()
    assert st[0, 0] == pytest.approx(0.5 / 440) and st[2, 0] == pytest.approx(170 / 10)
    st = U.metrics_update(st, sc, sf, np.array([0.5, 0.25]), (2, 11, 20, 1))
    assert st[0, 0] == pytest.approx(0.5 / 440 + 0.5) and st[3, 1] == 2 and st[4, 1] == 4
