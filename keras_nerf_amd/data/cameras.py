"""CameraModel -- calibrated cameras in front of the ray stage (csrc/rays_cam.hip): full intrinsics, OpenCV
radial / tangential distortion, the equidistant fisheye; one camera for a dataset or one per view.  Extension, no reference counterpart.

Conventions (include/knerf.h): normalised image coordinates with y pointing down, xn = (x + pixel_offset - cx) / fx for the integer
pixel x; the camera looks along -z with y up, as every pose of this project.  `pixel_offset` 0 puts a pixel's ray through its corner
(the plain camera of RaysGenerator), 0.5 through its centre (COLMAP, nerfstudio).  The kernels undistort with a fixed number of Newton
steps and cannot refuse a bad table without a synchronisation, so `check_invertible` establishes on the host, in fp64, that the
values are finite, the focal lengths positive and that the lens does not fold inside the image."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib

N_COEFFS = {"pinhole": 0, "opencv": 5, "fisheye": 4}      # opencv: k1, k2, p1, p2, k3; fisheye: k1, k2, k3, k4
NEWTON_STEPS = 8                                           # csrc/rays_cam.h kCamNewtonSteps


def opencv_distort(c, x, y):
    """OpenCV's distortion of normalised coordinates x, y [...] under c = (k1, k2, p1, p2, k3) [..., 5], fp64:
    (fx, fy, jacobian [..., 2, 2])"""
    k1, k2, p1, p2, k3 = (c[..., i] for i in range(5))
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    dr = k1 + r2 * (2.0 * k2 + 3.0 * k3 * r2)
    fx = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    fy = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    off = 2.0 * dr * x * y + 2.0 * (p1 * x + p2 * y)
    jac = np.stack([np.stack([rad + 2.0 * dr * x * x + 2.0 * p1 * y + 6.0 * p2 * x, off], -1),
                    np.stack([off, rad + 2.0 * dr * y * y + 6.0 * p1 * y + 2.0 * p2 * x], -1)], -2)
    return fx, fy, jac


def opencv_undistort(c, xn, yn, steps=NEWTON_STEPS):
    """the kernels' solve in fp64: `steps` Newton iterations from (xn, yn)"""
    x, y = np.array(xn, np.float64), np.array(yn, np.float64)
    for _ in range(steps):
        fx, fy, j = opencv_distort(c, x, y)
        ex, ey = fx - xn, fy - yn
        det = j[..., 0, 0] * j[..., 1, 1] - j[..., 0, 1] * j[..., 1, 0]
        x, y = x - (j[..., 1, 1] * ex - j[..., 0, 1] * ey) / det, y - (j[..., 0, 0] * ey - j[..., 1, 0] * ex) / det
    return x, y


def fisheye_distort(c, th):
    """theta_d and d theta_d / d theta of the equidistant fisheye under c = (k1, k2, k3, k4) [..., 4], fp64"""
    k1, k2, k3, k4 = (c[..., i] for i in range(4))
    t2 = th * th
    return (th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))),
            1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * 9.0 * k4))))


def fisheye_undistort(c, thd, steps=NEWTON_STEPS):
    th = np.array(thd, np.float64)
    for _ in range(steps):
        f, slope = fisheye_distort(c, th)
        th = th - (f - thd) / slope
    return th


class CameraModel:
    def __init__(self, model: str = "pinhole", fx=None, fy=None, cx=None, cy=None, distortion=(), pixel_offset: float = 0.0):
        """fx, fy, cx, cy: scalars or [V] arrays (pixels); distortion: [k] or [V,k], k up to 5 (opencv: k1, k2, p1, p2, k3) or 4
        (fisheye: k1, k2, k3, k4), missing trailing coefficients are 0.  Every per-view argument must have the same V."""
        if model not in _lib.CAMERA_MODELS:
            raise ValueError(f"model = {model!r}: expected one of {sorted(_lib.CAMERA_MODELS)}")
        if any(v is None for v in (fx, fy, cx, cy)):
            raise ValueError("fx, fy, cx and cy are all required")
        self.model, self.pixel_offset = model, float(pixel_offset)
        vals = [np.atleast_1d(np.asarray(v, np.float64)) for v in (fx, fy, cx, cy)]
        dist = np.asarray(distortion, np.float64)
        dist = dist.reshape(1, -1) if dist.ndim <= 1 else dist
        if any(v.ndim != 1 for v in vals) or dist.ndim != 2:
            raise ValueError("fx, fy, cx, cy are scalars or [V] arrays and distortion is [k] or [V,k]")
        if dist.shape[1] > N_COEFFS[model]:
            raise ValueError(f"a {model} camera takes at most {N_COEFFS[model]} distortion coefficients, got {dist.shape[1]}")
        counts = {len(v) for v in vals} | {dist.shape[0]}
        if len(counts - {1}) > 1:
            raise ValueError(f"per-view arguments of different lengths: {sorted(counts)}")
        n = max(counts)
        self.fx, self.fy, self.cx, self.cy = (np.broadcast_to(v, (n,)).copy() for v in vals)
        self.distortion = np.zeros((n, N_COEFFS[model]))
        self.distortion[:, :dist.shape[1]] = dist
        self._dev = {}

    @classmethod
    def from_focal(cls, focal: float, W: int, H: int) -> "CameraModel":
        """the plain camera of RaysGenerator(focal, W, H): rays through the pixel corners, principal point at the image centre"""
        return cls("pinhole", focal, focal, W * 0.5, H * 0.5, pixel_offset=0.0)

    @property
    def n_cameras(self) -> int:
        return len(self.fx)

    def _with(self, fx, fy, cx, cy, distortion) -> "CameraModel":
        return CameraModel(self.model, fx, fy, cx, cy, distortion, self.pixel_offset)

    def scaled(self, sx: float, sy: float) -> "CameraModel":
        """the camera of the same photographs resized by sx horizontally and sy vertically (normalised coordinates are unchanged)"""
        return self._with(self.fx * sx, self.fy * sy, self.cx * sx, self.cy * sy, self.distortion)

    def select(self, view_indices) -> "CameraModel":
        """the cameras of these views, in this order; a shared camera stays shared"""
        if self.n_cameras == 1:
            return self
        i = np.asarray(view_indices, np.int64).reshape(-1)
        if i.size and (i.min() < 0 or i.max() >= self.n_cameras):
            raise ValueError(f"view indices outside [0, {self.n_cameras})")
        return self._with(self.fx[i], self.fy[i], self.cx[i], self.cy[i], self.distortion[i])

    def table(self) -> np.ndarray:
        """float32 [C,12]: fx, fy, cx, cy, the coefficients, zeros (include/knerf.h)"""
        t = np.zeros((self.n_cameras, _lib.CAMERA_ROW), np.float32)
        t[:, 0], t[:, 1], t[:, 2], t[:, 3] = self.fx, self.fy, self.cx, self.cy
        t[:, 4:4 + self.distortion.shape[1]] = self.distortion
        return t

    def c_struct(self) -> "_lib.KnerfCameraModel":
        return _lib.KnerfCameraModel(_lib.CAMERA_MODELS[self.model], self.pixel_offset)

    def device_table(self, device="cuda"):
        """table() on the device, uploaded once per device"""
        import torch
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = torch.as_tensor(self.table()).to(device)
        return self._dev[device]

    # ---- host-side validation
    def check_invertible(self, W: int, H: int, sweep: int = 64) -> dict:
        """Raises ValueError unless every value is finite, fx, fy > 0 and the lens is invertible over the W x H image: for every
        border pixel of every camera the fp64 mirror of the kernels' 8-step Newton solve must land on the pixel (residual <= 1e-7 in
        normalised coordinates, below what fp32 resolves) and the distortion Jacobian must keep det > 0 (fisheye: d theta_d / d theta
        > 0, and theta < pi) along the sweep from the principal point to the solution.  Returns the smallest determinant (slope) and
        the largest residual seen."""
        t = np.concatenate([self.fx, self.fy, self.cx, self.cy, self.distortion.reshape(-1), [self.pixel_offset]])
        if not np.all(np.isfinite(t)):
            raise ValueError("the camera holds non-finite values")
        if not (np.all(self.fx > 0) and np.all(self.fy > 0)):
            raise ValueError(f"focal lengths must be positive, got fx = {self.fx.min()}, fy = {self.fy.min()}")
        if W <= 0 or H <= 0:
            raise ValueError(f"an image of {W} x {H} pixels")
        out = {"min_det": 1.0, "max_residual": 0.0}
        if self.model == "pinhole":
            return out
        xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        border = (xs == 0) | (xs == W - 1) | (ys == 0) | (ys == H - 1)
        px, py = xs[border] + self.pixel_offset, ys[border] + self.pixel_offset                   # [P]
        xn = (px[None] - self.cx[:, None]) / self.fx[:, None]                                     # [C,P]
        yn = (py[None] - self.cy[:, None]) / self.fy[:, None]
        c = self.distortion[:, None, :]
        s = np.linspace(0.0, 1.0, sweep)[:, None, None]
        with np.errstate(all="ignore"):
            if self.model == "opencv":
                xu, yu = opencv_undistort(c, xn, yn)
                fx, fy, _ = opencv_distort(c, xu, yu)
                res = np.hypot(fx - xn, fy - yn)
                j = opencv_distort(c[None], s * xu[None], s * yu[None])[2]
                det = j[..., 0, 0] * j[..., 1, 1] - j[..., 0, 1] * j[..., 1, 0]
                what = "the distortion Jacobian's determinant"
            else:
                thd = np.hypot(xn, yn)
                th = fisheye_undistort(c, thd)
                res = np.abs(fisheye_distort(c, th)[0] - thd)
                det = fisheye_distort(c[None], s * th[None])[1]
                what = "d theta_d / d theta"
                if np.all(np.isfinite(th)) and th.max() >= np.pi:
                    raise ValueError(f"the fisheye lens reaches theta = {th.max():.3f} >= pi inside the {W} x {H} image")
        if not (np.all(np.isfinite(res)) and np.all(np.isfinite(det))) or res.max() > 1e-7:
            raise ValueError(f"the lens is not invertible inside the {W} x {H} image: {NEWTON_STEPS} Newton steps leave a residual of "
                             f"{np.nanmax(res):.3g} (normalised coordinates) at a border pixel -- the distortion folds before the border")
        if det.min() <= 0:
            raise ValueError(f"the lens folds inside the {W} x {H} image: {what} falls to {det.min():.3g} on the way to a border pixel")
        return {"min_det": float(det.min()), "max_residual": float(res.max())}

    # ---- the forward map on the device
    def project(self, points, c2w, view=None):
        """knerf_project_points: world points [n,3] seen from camera `view[i]` (int [n]; None: view 0) of poses c2w [V,4,4] ->
        (pixels [n,2] in the coordinates the ray kernels take, depth [n], valid [n] bool), on the device.  A per-view camera needs
        V = n_cameras."""
        import torch
        from ..runtime import KnerfError
        if not torch.cuda.is_available():
            raise KnerfError("keras_nerf_amd needs an MI355X (gfx950) GPU; there is no CPU path")
        f32 = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, np.float32))).to("cuda", torch.float32).contiguous()
        pts, M = f32(points).reshape(-1, 3), f32(c2w).reshape(-1, 4, 4)
        n, V = pts.shape[0], M.shape[0]
        if n == 0:
            raise ValueError("no points")
        if self.n_cameras not in (1, V):
            raise ValueError(f"{self.n_cameras} cameras for {V} views")
        vw = None
        if view is not None:
            vw = (view if isinstance(view, torch.Tensor) else torch.as_tensor(np.asarray(view))).to("cuda", torch.int32).reshape(-1).contiguous()
            if vw.shape[0] != n:
                raise ValueError(f"{vw.shape[0]} view indices for {n} points")
            if int(vw.min()) < 0 or int(vw.max()) >= V:              # the kernel indexes c2w with them
                raise ValueError(f"view indices outside [0, {V})")
        pixels = torch.empty((n, 2), device=pts.device); depth = torch.empty((n,), device=pts.device)
        valid = torch.empty((n,), device=pts.device, dtype=torch.uint8)
        lib = _lib.load()
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        cam = self.c_struct()
        rc = lib.knerf_project_points(C.c_void_p(torch.cuda.current_stream(pts.device).cuda_stream), p(pts), p(vw), p(M),
                                      p(self.device_table(pts.device)), self.n_cameras, C.byref(cam), n, p(pixels), p(depth), p(valid))
        if rc != 0:
            msg = f"knerf_project_points failed ({rc}): {lib.knerf_last_error(None).decode(errors='replace')}"
            raise ValueError(msg) if rc == _lib.KNERF_ERR_INVALID else KnerfError(msg)
        return pixels, depth, valid.bool()
