"""fp64 NumPy restatements of the camera models (include/knerf.h, csrc/rays_cam.h) -- OpenCV distortion, its
30-step Newton inverse, the equidistant fisheye, the camera ray and the projection: the specifications the kernels are tested against.
Written from the formulas of the header, not from the product's Python.  Plus a float32 mirror of the kernels' 8-step arithmetic (every
operation a separate float32 NumPy op, one rounding each, in the kernels' order) and the camera sets the tests share."""
import numpy as np

V, H, W, N = 3, 12, 20, 8
# name -> (model, fx, fy, cx, cy, coefficients): opencv k1, k2, p1, p2, k3; fisheye k1, k2, k3, k4
SETS = {
    "intrinsics": ("pinhole", 18.0, 17.0, 10.3, 5.6, ()),
    "mild": ("opencv", 18.0, 17.0, 10.3, 5.6, (-0.12, 0.03, 0.002, -0.003, -0.004)),
    "strong": ("opencv", 11.0, 10.5, 9.4, 6.3, (-0.25, 0.07, 0.004, -0.005, -0.008)),
    "fisheye": ("fisheye", 7.0, 6.8, 9.6, 6.2, (-0.04, 0.01, -0.003, 0.0005)),
    "fisheye_wide": ("fisheye", 4.5, 4.4, 9.6, 6.2, (-0.03, 0.006, -0.001, 0.0001)),
}
OFFSETS = (0.0, 0.5)
KERNEL_STEPS = 8
# the GPU bounds of tests/test_gpu_cameras.py; the float32 mirror must stay within a fifth of each (tests/test_cameras_host.py)
BOUND_DIRECTION, BOUND_UNIT, BOUND_ROUND_TRIP_PX, BOUND_DEPTH_REL = 2e-6, 1e-6, 1e-4, 1e-5


def pixel_grid(offset, dtype=np.float64):
    """(x, y) [H,W]: the integer pixel coordinates plus the offset"""
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    return x.astype(dtype) + dtype(offset), y.astype(dtype) + dtype(offset)


# ---- fp64
def distort(c, x, y):
    k1, k2, p1, p2, k3 = c
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def distort_jacobian(c, x, y):
    """[..., 2, 2] by central differences of distort in fp64 (h = 1e-6): independent of the analytic Jacobian under test"""
    h = 1e-6
    ax, ay = distort(c, x + h, y)
    bx, by = distort(c, x - h, y)
    cx, cy = distort(c, x, y + h)
    dx, dy = distort(c, x, y - h)
    return np.stack([np.stack([(ax - bx), (cx - dx)], -1), np.stack([(ay - by), (cy - dy)], -1)], -2) / (2 * h)


def undistort(c, xn, yn, steps=30):
    """Newton on distort(x, y) = (xn, yn) from (xn, yn) with the analytic Jacobian"""
    k1, k2, p1, p2, k3 = c
    x, y = np.array(xn, np.float64), np.array(yn, np.float64)
    for _ in range(steps):
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        dr = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2
        a = rad + 2 * x * x * dr + 2 * p1 * y + 6 * p2 * x
        b = 2 * x * y * dr + 2 * p1 * x + 2 * p2 * y
        d = rad + 2 * y * y * dr + 6 * p1 * y + 2 * p2 * x
        fx, fy = distort(c, x, y)
        ex, ey = fx - xn, fy - yn
        det = a * d - b * b
        x, y = x - (d * ex - b * ey) / det, y - (a * ey - b * ex) / det
    return x, y


def fisheye_theta_d(c, th):
    k1, k2, k3, k4 = c
    return th * (1 + k1 * th ** 2 + k2 * th ** 4 + k3 * th ** 6 + k4 * th ** 8)


def fisheye_slope(c, th):
    k1, k2, k3, k4 = c
    return 1 + 3 * k1 * th ** 2 + 5 * k2 * th ** 4 + 7 * k3 * th ** 6 + 9 * k4 * th ** 8


def fisheye_theta(c, thd, steps=30):
    th = np.array(thd, np.float64)
    for _ in range(steps):
        th = th - (fisheye_theta_d(c, th) - thd) / fisheye_slope(c, th)
    return th


def normalised(cam, offset):
    """(xn, yn) [H,W] of every pixel"""
    _, fx, fy, cx, cy, _ = cam
    x, y = pixel_grid(offset)
    return (x - cx) / fx, (y - cy) / fy


def camera_vectors(cam, offset, steps=30):
    """[H,W,3]: the camera-space vector of every pixel (not normalised for pinhole / opencv)"""
    model, c = cam[0], cam[5]
    xn, yn = normalised(cam, offset)
    if model == "fisheye":
        thd = np.hypot(xn, yn)
        th = fisheye_theta(c, thd, steps)
        s = np.where(thd > 0, np.sin(th) / np.where(thd > 0, thd, 1.0), 0.0)
        return np.stack([s * xn, -s * yn, np.where(thd > 0, -np.cos(th), -1.0)], -1)
    xu, yu = undistort(c, xn, yn, steps) if model == "opencv" else (xn, yn)
    return np.stack([xu, -yu, -np.ones_like(xu)], -1)


def camera_rays(cam, offset, c2w):
    """(o [V,H,W,3], unit d [V,H,W,3]) in fp64"""
    c2w = np.asarray(c2w, np.float64)
    v = camera_vectors(cam, offset)
    d = np.einsum("vrc,hwc->vhwr", c2w[:, :3, :3], v)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.broadcast_to(c2w[:, None, None, :3, 3], d.shape).copy(), d


def project(cam, offset, c2w, points):
    """points [V,...,3] seen from view v of c2w [V,4,4] -> (pixels [V,...,2], depth [V,...], valid [V,...]) in fp64"""
    model, fx, fy, cx, cy, c = cam
    c2w, points = np.asarray(c2w, np.float64), np.asarray(points, np.float64)
    q = points - c2w[:, :3, 3].reshape((len(c2w),) + (1,) * (points.ndim - 2) + (3,))
    p = np.einsum("vrc,v...r->v...c", c2w[:, :3, :3], q)
    depth = -p[..., 2]
    with np.errstate(all="ignore"):
        if model == "fisheye":
            r = np.hypot(p[..., 0], p[..., 1])
            th = np.arctan2(r, depth)
            s = np.where(r > 0, fisheye_theta_d(c, th) / np.where(r > 0, r, 1.0), 0.0)
            xn, yn = s * p[..., 0], -s * p[..., 1]
            valid = ((r > 0) | (depth > 0)) & (th < np.pi)
        else:
            xu, yu = p[..., 0] / depth, -p[..., 1] / depth
            xn, yn = distort(c, xu, yu) if model == "opencv" else (xu, yu)
            valid = depth > 0
    return np.stack([xn * fx + cx - offset, yn * fy + cy - offset], -1), depth, valid


# ---- float32, the kernels' order of operations (csrc/rays_cam.h)
F = np.float32


def _poly32(t2, coeffs):
    """1 + t2 (c0 + t2 (c1 + ...)) in float32"""
    acc = F(coeffs[-1]) * np.ones_like(t2)
    for k in coeffs[-2::-1]:
        acc = F(k) + t2 * acc
    return F(1) + t2 * acc


def distort32(c, x, y, jac=False):
    k1, k2, p1, p2, k3 = (F(v) for v in c)
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    rad = F(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
    fx = (x * rad + (F(2) * p1) * xy) + p2 * (r2 + F(2) * xx)
    fy = (y * rad + p1 * (r2 + F(2) * yy)) + (F(2) * p2) * xy
    if not jac:
        return fx, fy
    dr2 = F(2) * (k1 + r2 * (F(2) * k2 + (F(3) * k3) * r2))
    off = dr2 * xy + F(2) * (p1 * x + p2 * y)
    a = (rad + dr2 * xx) + ((F(2) * p1) * y + (F(6) * p2) * x)
    d = (rad + dr2 * yy) + ((F(6) * p1) * y + (F(2) * p2) * x)
    return fx, fy, a, off, d


def undistort32(c, xn, yn, steps=KERNEL_STEPS):
    x, y = xn.copy(), yn.copy()
    for _ in range(steps):
        fx, fy, a, b, d = distort32(c, x, y, jac=True)
        ex, ey = fx - xn, fy - yn
        det = a * d - b * b
        x, y = x - (d * ex - b * ey) / det, y - (a * ey - b * ex) / det
    return x, y


def fisheye_theta_d32(c, th):
    return th * _poly32(th * th, c)


def fisheye_theta32(c, thd, steps=KERNEL_STEPS):
    th = thd.copy()
    odd = [F(3) * F(c[0]), F(5) * F(c[1]), F(7) * F(c[2]), F(9) * F(c[3])]
    for _ in range(steps):
        th = th - (fisheye_theta_d32(c, th) - thd) / _poly32(th * th, odd)
    return th


def normalised32(cam, offset, steps=KERNEL_STEPS):
    """float32 (xn, yn, xu, yu): distorted and, for opencv, undistorted normalised coordinates of every pixel (fisheye: xu = theta)"""
    model, fx, fy, cx, cy, c = cam
    x, y = pixel_grid(offset, np.float32)
    xn, yn = (x - F(cx)) / F(fx), (y - F(cy)) / F(fy)
    if model == "opencv":
        return (xn, yn) + undistort32(c, xn, yn, steps)
    if model == "fisheye":
        return xn, yn, fisheye_theta32(c, np.sqrt(xn * xn + yn * yn), steps), None
    return xn, yn, xn, yn


def camera_rays32(cam, offset, c2w, steps=KERNEL_STEPS):
    """(o, d) [V,H,W,3] float32 with the kernels' roundings"""
    xn, yn, xu, yu = normalised32(cam, offset, steps)
    if cam[0] == "fisheye":
        thd, th = np.sqrt(xn * xn + yn * yn), xu
        with np.errstate(all="ignore"):
            s = np.where(thd > 0, np.sin(th) / thd, F(0)).astype(np.float32)
        v = [s * xn, -(s * yn), np.where(thd > 0, -np.cos(th), F(-1)).astype(np.float32)]
    else:
        v = [xu, -yu, np.full_like(xu, -1)]
    M = np.asarray(c2w, np.float32)
    dv = [(v[0][None] * M[:, r, 0, None, None] + v[1][None] * M[:, r, 1, None, None]) + v[2][None] * M[:, r, 2, None, None] for r in range(3)]
    nrm = np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
    d = np.stack([q / nrm for q in dv], -1)
    return np.broadcast_to(M[:, None, None, :3, 3], d.shape).copy(), d


def project32(cam, offset, c2w, points):
    """points [V,...,3] float32 -> (pixels, depth, valid) with the projection kernel's roundings"""
    model, fx, fy, cx, cy, c = cam
    M, points = np.asarray(c2w, np.float32), np.asarray(points, np.float32)
    shape = (len(M),) + (1,) * (points.ndim - 2)
    q = [points[..., r] - M[:, r, 3].reshape(shape) for r in range(3)]
    p = [(M[:, 0, k].reshape(shape) * q[0] + M[:, 1, k].reshape(shape) * q[1]) + M[:, 2, k].reshape(shape) * q[2] for k in range(3)]
    depth = -p[2]
    with np.errstate(all="ignore"):
        if model == "fisheye":
            r = np.sqrt(p[0] * p[0] + p[1] * p[1])
            th = np.arctan2(r, depth)
            s = np.where(r > 0, fisheye_theta_d32(c, th) / r, F(0)).astype(np.float32)
            xn, yn = s * p[0], -(s * p[1])
            valid = ((r > 0) | (depth > 0)) & (th < F(np.pi))
        else:
            xu, yu = p[0] / depth, -(p[1] / depth)
            xn, yn = distort32(c, xu, yu) if model == "opencv" else (xu, yu)
            valid = depth > 0
    return np.stack([(xn * F(fx) + F(cx)) - F(offset), (yn * F(fy) + F(cy)) - F(offset)], -1), depth, valid
