"""csrc/utils_ops.hip at the limits its own argument checks admit, one op at a time against tests/utils_ops_reference.py and the oracle:
positional encoding for L = 0 ... 30 against float64 sin / cos of the kernel's float32 argument; knerf_inverse_cdf bit for bit up to
4,096 weights with any number of mid-points; knerf_ray_points bit for bit; PSNR and SSIM on thin images and on flat bright regions;
three consecutive knerf_metrics_update steps against float64 running means.  `pytest -s` prints the measured figures."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import utils_ops_reference as U

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def _lib():
    from keras_nerf_amd import _lib
    return _lib.load(), _lib.KNERF_ERR_INVALID


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def utils():
    from keras_nerf_amd.model.nerf.utils import NeRFUtils
    return NeRFUtils(1, 16, 16, 128, 10, 4)


# ---- positional encoding

@pytest.mark.parametrize("rows", U.POSENC_ROWS)
@pytest.mark.parametrize("L", U.POSENC_L)
def test_positional_encoding_against_float64(utils, L, rows):
    """Bound per case: max(2^-22, 4 x the deviation of NumPy's float32 sin / cos from float64 on the same arguments) = 2.4e-7 ... 2.5e-7.
    Measured on an MI355X: 0 for L = 0, 3.9e-8 ... 6.4e-8 otherwise (the worst at L = 30, arguments up to 2^29 x 1e3)."""
    lib, _ = _lib()
    x = U.posenc_inputs(rows)
    want, bound = U.posenc_float64(x, L), U.posenc_bound(x, L)
    got = utils.positional_encoding(x, L).cpu().numpy()
    dx = torch.as_tensor(x, device="cuda")
    out = torch.full((rows, 3 + 6 * L), -7.0, device="cuda")
    assert lib.knerf_positional_encoding(_stream(), _p(dx), rows, L, _p(out)) == 0
    assert got.shape == (rows, 3 + 6 * L) and np.array_equal(out.cpu().numpy().view(np.uint32), got.view(np.uint32))
    assert np.array_equal(got[:, :3].view(np.uint32), x.view(np.uint32))                       # signed zeros included
    err = float(np.abs(got.astype(f64) - want).max())
    print(f"posenc L {L} rows {rows}: error {err:.2e}, bound {bound:.2e}")
    assert np.isfinite(got).all() and err <= bound


def test_positional_encoding_refuses_depths_outside_0_30(utils):
    lib, INVALID = _lib()
    x = torch.zeros((4, 3), device="cuda")
    out = torch.full((4, 3 + 6 * 31), -7.0, device="cuda")
    for L in (31, -1):
        assert lib.knerf_positional_encoding(_stream(), _p(x), 4, L, _p(out)) == INVALID
    assert (out == -7).all()
    with pytest.raises(ValueError):
        utils.positional_encoding(np.zeros((4, 3), f32), 31)


# ---- inverse cdf

def _inverse_cdf(lib, mids, w, u, clamp):
    dm, dw, du = (torch.as_tensor(a, device="cuda") for a in (mids, w, u))
    out = torch.full(u.shape, -7.0, device="cuda")
    rc = lib.knerf_inverse_cdf(_stream(), _p(dm), _p(dw), _p(du), len(w), mids.shape[1], w.shape[1], u.shape[1], int(clamp), _p(out))
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("n_samples", U.INVERSE_CDF_SAMPLES)
@pytest.mark.parametrize("rays", U.INVERSE_CDF_RAYS)
@pytest.mark.parametrize("n_weights,n_mid", U.INVERSE_CDF_SHAPES)
def test_inverse_cdf_bit_exact(n_weights, n_mid, rays, n_samples):
    """n_mid unrelated to n_weights; 1 and 5 rays (a workgroup holds four: waves without a ray); 4,096 weights = 65,552 bytes of
    dynamic LDS, 16 past 64 KiB: the MI355X launches it (return code 0, every value exact), so 4,096 stays the documented limit"""
    lib, _ = _lib()
    mids, w, u = U.inverse_cdf_inputs(n_weights, n_mid, rays, n_samples)
    for oob in ("zero", "clamp"):
        rc, got = _inverse_cdf(lib, mids, w, u, oob == "clamp")
        assert rc == 0, rc
        np.testing.assert_array_equal(got, O.fine_hierarchical_sampling_chunk(mids, w, u, oob))


def test_inverse_cdf_refuses_4097_weights():
    lib, INVALID = _lib()
    mids, w, u = U.inverse_cdf_inputs(4097, 4096, 1, 1)
    rc, got = _inverse_cdf(lib, mids, w, u, False)
    assert rc == INVALID and (got == -7).all()


# ---- ray points

@pytest.mark.parametrize("rays,samples", U.RAY_POINT_SHAPES)
def test_ray_points_bit_exact(rays, samples):
    lib, _ = _lib()
    rng = np.random.default_rng(rays)
    o, d = rng.normal(0, 1, (rays, 3)).astype(f32), rng.normal(0, 1, (rays, 3)).astype(f32)
    t = rng.uniform(2, 6, (rays, samples)).astype(f32)
    do, dd, dt = (torch.as_tensor(a, device="cuda") for a in (o, d, t))
    out = torch.full((rays, samples, 3), -7.0, device="cuda")
    assert lib.knerf_ray_points(_stream(), _p(do), _p(dd), _p(dt), rays, samples, _p(out)) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint32), U.ray_points(o, d, t).view(np.uint32))


# ---- image metrics

@pytest.mark.parametrize("kind", U.METRIC_CLASSES)
@pytest.mark.parametrize("shape", U.METRIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_psnr_and_ssim_against_float64(shape, kind):
    """The project's bounds: PSNR rtol 1e-5, SSIM atol 2e-5.  Measured on an MI355X, |ssim - float64|, worst shape per class:

    | class | xx - mx mx on raw pixels (the kernel until this test) | moments about the window's centre pixel of A (now) |
    |---|---|---|
    | random | 6.0e-7 | 9.5e-7 (both on the one-window 11 x 11 image; 5.3e-8 on the others) |
    | A = 0.95, B = A + 1e-3 noise | **5.6e-4** | 7.1e-8 |
    | A = 0.5, B = A + 1e-2 noise | 1.3e-5 | 1.3e-7 |
    | both 0.95 + 1e-3 noise | **1.8e-4** | 6.0e-8 |
    | white with a textured patch | **5.2e-5** | 3.5e-7 (11 x 11; 7.3e-8 on the others) |
    | A = B | 0 | 0 |

    The left column is the float32 plain mirror of tests/test_utils_ops_host.py to two digits, the right one its pivoted mirror.
    PSNR: 1.4e-7 relative at the worst."""
    from keras_nerf_amd.model.nerf.metrics import psnr, ssim
    a, b = U.metric_images(kind, shape)
    ta, tb = torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda")
    with np.errstate(divide="ignore"):
        want_p, want_s = O.psnr(a, b), O.ssim(a, b)
    got_p, got_s = psnr(ta, tb).cpu().numpy(), ssim(ta, tb).cpu().numpy()
    print(f"{shape} {kind}: ssim error {np.abs(got_s - want_s).max():.2e}, "
          f"psnr relative error {np.abs(got_p / want_p - 1).max() if np.isfinite(want_p).all() else 0.0:.2e}")
    np.testing.assert_allclose(got_p, want_p, rtol=U.PSNR_RTOL)
    np.testing.assert_allclose(got_s, want_s, atol=U.SSIM_ATOL, rtol=0)
    np.testing.assert_allclose(ssim(ta, ta).cpu().numpy(), 1.0, atol=1e-5, rtol=0)
    if kind == "same":
        assert (got_p == np.inf).all()


# ---- running means

@pytest.mark.parametrize("with_loss", [True, False])
@pytest.mark.parametrize("n_images", [1, 3])
def test_three_metric_updates_against_float64(n_images, with_loss):
    """Three steps on one MetricState.  Reference: float64 totals from the device's own two sums per image (one workgroup per image
    at this size, so a second launch gives the same bits), so only metrics_update_kernel's arithmetic is under test: its float32
    ratios and log10f stay within 1e-6 relative; counts are exact.  Measured on an MI355X: 4.0e-8 at the worst (a PSNR total)."""
    from keras_nerf_amd.model.nerf.metrics import MetricState, _image_sums
    shape = (n_images, 16, 21, 3)
    ms = MetricState(torch.device("cuda"))
    want = np.zeros((6, 2))
    for step in range(3):
        img, coarse = U.metric_images("random", shape, seed=10 + step)
        _, fine = U.metric_images("flat_05_1e-2", shape, seed=20 + step)
        fine = np.clip(img + (fine - f32(0.5)), 0, 1).astype(f32)
        ti, tc, tf = (torch.as_tensor(z, device="cuda") for z in (img, coarse, fine))
        loss = np.array([0.25 / (step + 1), 0.125 + step], f32) if with_loss else None
        ms.update(ti, tc, tf, None if loss is None else torch.as_tensor(loss, device="cuda"))
        sc, sf = (_image_sums(ti, z)[0].cpu().numpy() for z in (tc, tf))
        want = U.metrics_update(want, sc, sf, loss, shape)
    got = ms.state.cpu().numpy()
    assert np.array_equal(got[:, 1], want[:, 1]) and got[:, 1].tolist() == [3, 3 * n_images, 3 * n_images] * 2
    rel = np.abs(got[:, 0] / want[:, 0] - 1)
    print(f"metrics_update n_images {n_images} loss {with_loss}: relative error of the six totals {rel}")
    assert (rel <= 1e-6).all()


@pytest.mark.parametrize("with_loss", [True, False])
def test_identical_image_gives_an_infinite_psnr_total(with_loss):
    """A = B in one image of the batch: PSNR +inf like tf.image.psnr, not NaN; the SSIM and loss rows stay finite"""
    from keras_nerf_amd.model.nerf.metrics import MetricState
    shape = (3, 16, 21, 3)
    img, coarse = U.metric_images("random", shape, seed=1)
    _, fine = U.metric_images("random", shape, seed=1)
    coarse[1] = img[1]
    ms = MetricState(torch.device("cuda"))
    loss = torch.tensor([0.5, 0.25], device="cuda") if with_loss else None
    ms.update(*(torch.as_tensor(z, device="cuda") for z in (img, coarse, fine)), loss)
    got = ms.state.cpu().numpy()
    assert got[1, 0] == np.inf and np.isfinite(got[[0, 2, 3, 4, 5], 0]).all()
    assert got[:, 1].tolist() == [1, 3, 3, 1, 3, 3]
