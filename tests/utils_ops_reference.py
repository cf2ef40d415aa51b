"""NumPy references and case tables for csrc/utils_ops.hip (tests/test_utils_ops_host.py, tests/test_gpu_utils_ops.py): positional
encoding in float64 on the kernel's float32 arguments, ray points, the image classes of the metric tests, two float32 mirrors of
image_metrics_kernel's SSIM loop (plain and pivoted) and the running means of metrics_update_kernel in float64."""
import numpy as np

f32, f64 = np.float32, np.float64

# ---- positional encoding

POSENC_L = (0, 1, 10, 30)
POSENC_ROWS = (1, 85, 257)
POSENC_FLOOR = 2.0 ** -22


def posenc_inputs(rows):
    """[rows, 3] float32: |x| from 1e-3 to 1e3 with both signs, signed zeros, and multiples of pi/2 with their float32 neighbours"""
    if rows == 1:
        return np.array([[-0.0, np.nextafter(f32(np.pi / 2), f32(0)), 1e3]], f32)
    half_pi = np.array([f32(k * np.pi / 2) for k in range(1, 21)], f32)
    near = np.concatenate([half_pi, np.nextafter(half_pi, f32(0)), np.nextafter(half_pi, f32(100))])
    special = np.concatenate([np.array([-0.0, 0.0], f32), near, -near])                      # 122 values
    mags = np.logspace(-3, 3, 3 * rows - special.size).astype(f32)
    mags[1::2] *= f32(-1)
    x = np.concatenate([special, mags])
    return np.ascontiguousarray(x[np.random.default_rng(rows).permutation(x.size)].reshape(rows, 3))


def posenc_arguments(x, L):
    """[n, L, 3] float32: fl32(2^k x), the one rounding the kernel makes before sin / cos (exact unless the product is subnormal)"""
    x = np.asarray(x, f32).reshape(-1, 3)
    return (f32(2.0) ** np.arange(L, dtype=f32))[None, :, None] * x[:, None, :]


def _posenc(x, L, dt):
    x = np.asarray(x, f32).reshape(-1, 3)
    a = posenc_arguments(x, L).astype(dt)
    body = np.concatenate([np.sin(a), np.cos(a)], -1).reshape(len(x), 6 * L)       # per k: sin(3), cos(3)
    return np.concatenate([x.astype(dt), body], -1)


def posenc_float64(x, L):
    """[n, 3 + 6L] float64: x, then per k sin and cos of the float32 argument in float64"""
    return _posenc(x, L, f64)


def posenc_float32(x, L):
    """the same with NumPy's float32 sin / cos: its deviation from float64 is the yardstick for the device's sinf / cosf"""
    return _posenc(x, L, f32)


def posenc_bound(x, L):
    return max(POSENC_FLOOR, 4 * float(np.abs(posenc_float32(x, L).astype(f64) - posenc_float64(x, L)).max()))


# ---- inverse cdf, ray points

INVERSE_CDF_SHAPES = ((1, 1), (2, 1), (64, 1), (64, 67), (4096, 4095), (4096, 5000))          # (n_weights, n_mid)
INVERSE_CDF_RAYS = (1, 5)
INVERSE_CDF_SAMPLES = (1, 65)
RAY_POINT_SHAPES = ((1, 1), (3, 85), (257, 7))


def inverse_cdf_inputs(n_weights, n_mid, rays, n_samples):
    rng = np.random.default_rng(n_weights * 7 + n_mid * 3 + rays + n_samples)
    w = (rng.random((rays, n_weights)) ** 4).astype(f32)
    mids = np.sort(rng.uniform(2, 6, (rays, n_mid)).astype(f32), -1)
    u = rng.random((rays, n_samples), dtype=f32)
    u[0, 0] = 0.0
    u[-1, -1] = f32(1.0 - 2.0 ** -24)
    return mids, w, u


def ray_points(o, d, t):
    """o, d [R,3], t [R,S] -> [R,S,3] float32: the multiply and the add rounded separately"""
    prod = (d[:, None, :] * t[:, :, None]).astype(f32)
    return (o[:, None, :] + prod).astype(f32)


# ---- image metrics

METRIC_SHAPES = ((1, 11, 11, 1), (2, 11, 300, 3), (1, 300, 11, 3), (3, 37, 53, 4))
METRIC_CLASSES = ("random", "flat_095_1e-3", "flat_05_1e-2", "both_095_noise", "white_with_patch", "same")
FLAT_CLASSES = ("flat_095_1e-3", "flat_05_1e-2", "both_095_noise")
PSNR_RTOL, SSIM_ATOL = 1e-5, 2e-5


def metric_images(kind, shape, seed=0):
    rng = np.random.default_rng(seed)
    noise = lambda s: s * rng.standard_normal(shape).astype(f32)
    if kind == "random":
        a = rng.random(shape, dtype=f32)
        b = np.clip(a + noise(f32(0.1)), 0, 1)
    elif kind == "flat_095_1e-3":
        a = np.full(shape, 0.95, f32)
        b = np.clip(a + noise(f32(1e-3)), 0, 1)
    elif kind == "flat_05_1e-2":
        a = np.full(shape, 0.5, f32)
        b = np.clip(a + noise(f32(1e-2)), 0, 1)
    elif kind == "both_095_noise":
        a = np.clip(f32(0.95) + noise(f32(1e-3)), 0, 1)
        b = np.clip(f32(0.95) + noise(f32(1e-3)), 0, 1)
    elif kind == "white_with_patch":
        a = np.ones(shape, f32)
        a[:, :10, 1:11] = rng.random((shape[0], 10, 10, shape[3]), dtype=f32)
        b = np.clip(a + noise(f32(0.02)), 0, 1)
    elif kind == "same":
        a = rng.random(shape, dtype=f32)
        b = a.copy()
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)


def gauss11():
    """the window weights as knerf_image_metrics makes them: float64, normalised, rounded to float32"""
    k = np.arange(11, dtype=f64) - 5
    g = np.exp(-(k * k) / (2.0 * 1.5 * 1.5))
    return (g / g.sum()).astype(f32)


def ssim_mirror(a, b, pivot):
    """float32 mirror of image_metrics_kernel's window loop, all windows at once: [B] mean SSIM (the terms summed in float64, so the
    figure shows the loop's own error).  pivot False: the five sums of w x, w y, w x x, w y y, w x y, then xx - mx mx.  pivot True:
    the same sums of x - c and y - c with c the window's centre pixel of A in that channel; c goes back onto the means for the
    luminance term; variances and covariance are the same quantities, without the cancellation."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    B, H, W, C = a.shape
    h, w = H - 10, W - 10
    g = gauss11()
    c = a[:, 5:5 + h, 5:5 + w, :] if pivot else None
    mx = np.zeros((B, h, w, C), f32); my = mx.copy(); xx = mx.copy(); yy = mx.copy(); xy = mx.copy()
    for di in range(11):
        for dj in range(11):
            wt = f32(g[di] * g[dj])
            x, y = a[:, di:di + h, dj:dj + w, :], b[:, di:di + h, dj:dj + w, :]
            if pivot:
                x, y = x - c, y - c
            wx, wy = wt * x, wt * y
            mx += wx; my += wy; xx += wx * x; yy += wy * y; xy += wx * y
    sxx, syy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
    if pivot:
        mx, my = mx + c, my + c
    c1, c2 = f32(0.01) * f32(0.01), f32(0.03) * f32(0.03)
    term = (f32(2) * mx * my + c1) / (mx * mx + my * my + c1) * ((f32(2) * sxy + c2) / (sxx + syy + c2))
    assert term.dtype == f32
    return term.astype(f64).mean(axis=(1, 2, 3))


# ---- running means

def metrics_update(state, sums_coarse, sums_fine, loss, shape):
    """metrics_update_kernel in float64: state [6,2] {total, count} += one step.  sums [n,2] = the device's own {SSIM term sum, squared-
    difference sum} per image; loss [2] or None (test_step: the whole-batch mean squared error from the same sums)."""
    n, H, W, C = shape
    nwin, npix = (H - 10) * (W - 10) * C, H * W * C
    state = np.array(state, f64)
    with np.errstate(divide="ignore"):
        for k, s in enumerate((np.asarray(sums_coarse, f64), np.asarray(sums_fine, f64))):
            st = state[3 * k:3 * k + 3]
            st[0, 0] += float(loss[k]) if loss is not None else s[:, 1].sum() / (npix * n)
            st[0, 1] += 1
            st[1, 0] += (-10.0 * np.log10(s[:, 1] / npix)).sum()
            st[1, 1] += n
            st[2, 0] += (s[:, 0] / nwin).sum()
            st[2, 1] += n
    return state
