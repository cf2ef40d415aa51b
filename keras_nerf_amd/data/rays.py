"""RaysGenerator -- counterpart of reference keras_nerf/data/rays.py:4-130, generated on the GPU (csrc/raygen.hip).

Beyond the reference: `ndc=True` writes normalised-device-coordinate rays for forward-facing scenes and `spacing="disparity"` spaces
the samples of pinhole rays linearly in 1 / depth (csrc/rays_ext.hip).  With the defaults the plain entry
point is called exactly as before.  `camera=` (data/cameras.py CameraModel) replaces the single focal length by full intrinsics, lens
distortion or a fisheye, one camera or one per view (csrc/rays_cam.hip); without it nothing changes."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..runtime import KnerfError


class RaysGenerator:
    def __init__(self, focal_length: float, image_width: int, image_height: int, near: float, far: float, n_sample: int,
                 seed: int = 0, ndc: bool = False, ndc_near: float = 1.0, spacing: str = "linear", camera=None, **kwargs):
        """camera: None -- the pinhole camera of `focal_length` with its principal point at the image centre -- or a CameraModel, with
        which focal_length is not used and may be None; its table is checked on the host once (CameraModel.check_invertible)"""
        if camera is None and focal_length is None:
            raise ValueError("focal_length is required without a camera")
        self.focal_length = None if focal_length is None else float(focal_length)
        self.image_width, self.image_height, self.camera = int(image_width), int(image_height), camera
        self.near, self.far, self.n_sample = float(near), float(far), int(n_sample)
        self.seed, self._calls = seed, 0
        self.ndc, self.ndc_near, self.spacing = bool(ndc), float(ndc_near), spacing
        if spacing not in _lib.SPACINGS:
            raise ValueError(f"spacing = {spacing!r}: expected one of {sorted(_lib.SPACINGS)}")
        if not (np.isfinite(self.ndc_near) and self.ndc_near > 0):
            raise ValueError(f"ndc_near = {ndc_near}: the NDC near plane lies at a positive distance in front of the camera")
        if self.ndc and spacing == "disparity":
            raise ValueError("NDC rays are sampled linearly in NDC depth (already linear in disparity of the scene); "
                             "spacing='disparity' is for pinhole rays")
        if spacing == "disparity" and not self.near > 0:
            raise ValueError(f"spacing='disparity' needs near > 0, got {near}")
        if self.ndc and not 0 <= self.near <= self.far <= 1:
            raise ValueError(f"NDC rays take their samples at fractions of the ray: need 0 <= near <= far <= 1, got {near}, {far}")
        if camera is not None:
            if self.ndc and camera.model == "fisheye":
                raise ValueError("NDC rays need a camera that looks along -z: not the fisheye model")
            if self.ndc and camera.n_cameras > 1:
                raise ValueError("NDC rays take their scales from one camera, not from a per-view table")
            camera.check_invertible(self.image_width, self.image_height)
        if not torch.cuda.is_available():
            raise KnerfError("keras_nerf_amd needs an MI355X (gfx950) GPU; there is no CPU path")
        self._lib = _lib.load()

    @property
    def ray_model(self):
        """None for the plain rays (pinhole, samples linear in depth), else the struct knerf_ray_model of this generator"""
        if not self.ndc and self.spacing == "linear":
            return None
        return _lib.KnerfRayModel(int(self.ndc), _lib.SPACINGS[self.spacing], self.ndc_near)

    def __call__(self, camera_params, noise=None, view_index=None):
        """camera_params: 4x4 camera-to-world (or [B,4,4]).  Returns (ray_origin, ray_direction [...,H,W,3],
        sample_points [...,H,W,n_sample]); the jitter is redrawn on every call (rays.py:122-123) unless `noise` is given.
        view_index: with a per-view camera, which of its rows each of the B matrices takes (ints [B]; without it B must be the
        number of cameras, row v for matrix v)."""
        c2w = torch.as_tensor(np.asarray(camera_params, np.float32) if not isinstance(camera_params, torch.Tensor)
                              else camera_params).to("cuda", torch.float32).contiguous()
        single = c2w.dim() == 2
        c2w = c2w.reshape(-1, 4, 4)
        B, H, W, N = c2w.shape[0], self.image_height, self.image_width, self.n_sample
        nz = None if noise is None else torch.as_tensor(np.asarray(noise, np.float32) if not isinstance(noise, torch.Tensor)
                                                        else noise).to("cuda", torch.float32).reshape(B, H, W, N).contiguous()
        o = torch.empty((B, H, W, 3), device="cuda"); d = torch.empty_like(o); t = torch.empty((B, H, W, N), device="cuda")
        self._calls += 1
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        model = self.ray_model
        if self.camera is not None:
            return self._call_cam(c2w, nz, o, d, t, model, view_index, single)
        if view_index is not None:
            raise ValueError("view_index is for a generator with a per-view camera")
        if model is None:
            rc = self._lib.knerf_generate_rays(None, C.c_void_p(torch.cuda.current_stream().cuda_stream), p(c2w), p(nz), self.seed,
                                               self._calls, B, H, W, N, self.focal_length, self.near, self.far, p(o), p(d), p(t))
        else:
            rc = self._lib.knerf_generate_rays_ext(None, C.c_void_p(torch.cuda.current_stream().cuda_stream), p(c2w), p(nz), self.seed,
                                                   self._calls, B, H, W, N, self.focal_length, self.near, self.far, p(o), p(d), p(t),
                                                   C.byref(model))
        if rc != 0:
            raise KnerfError(f"knerf_generate_rays{'' if model is None else '_ext'} failed ({rc}): "
                             f"{self._lib.knerf_last_error(None).decode(errors='replace')}")
        return (o[0], d[0], t[0]) if single else (o, d, t)

    def _call_cam(self, c2w, nz, o, d, t, model, view_index, single):
        cam = self.camera
        B, H, W, N = t.shape
        table = cam.device_table(c2w.device)
        if cam.n_cameras > 1:
            if view_index is None:
                if B != cam.n_cameras:
                    raise ValueError(f"{B} camera matrices for a table of {cam.n_cameras} cameras: pass view_index")
            else:
                sel = (view_index if isinstance(view_index, torch.Tensor) else torch.as_tensor(np.asarray(view_index, np.int64)))
                sel = sel.to(c2w.device, torch.int64).reshape(-1)
                if sel.shape[0] != B:
                    raise ValueError(f"{sel.shape[0]} view indices for {B} camera matrices")
                if not isinstance(view_index, torch.Tensor) and B and not 0 <= int(np.min(view_index)) <= int(np.max(view_index)) < cam.n_cameras:
                    raise ValueError(f"view indices outside [0, {cam.n_cameras})")
                table = table.index_select(0, sel).contiguous()
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        cs = cam.c_struct()
        rc = self._lib.knerf_generate_rays_cam(None, C.c_void_p(torch.cuda.current_stream().cuda_stream), p(c2w), p(nz), self.seed,
                                               self._calls, B, H, W, N, p(table), table.shape[0], C.byref(cs), self.near, self.far,
                                               p(o), p(d), p(t), None if model is None else C.byref(model))
        if rc != 0:
            raise KnerfError(f"knerf_generate_rays_cam failed ({rc}): {self._lib.knerf_last_error(None).decode(errors='replace')}")
        return (o[0], d[0], t[0]) if single else (o, d, t)
