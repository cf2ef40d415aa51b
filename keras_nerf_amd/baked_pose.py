"""Refining camera poses against a baked field (extension, no reference counterpart; BARF, NeRF-- and the current toolkits optimise
their cameras together with the field, because structure-from-motion poses are off by fractions of a degree and no amount of field
training removes the blur that causes).

The arithmetic on the rays is HIP (csrc/baked_pose.hip: knerf_baked_ray_gradients[_bricks] gives the gradient of the baked-field
objective with respect to every ray's origin and direction, knerf_pose_gradients sums those to one rigid-motion gradient per camera;
include/knerf.h holds the contract, DESIGN.md 2.24 the derivation).  The pose state is V x 18 numbers: its Adam step and the
Rodrigues update are plain torch on the device.  No step waits for the GPU.

Not covered: the MLP path has no input gradient; NDC rays are refused (the pose does not enter them as o = t, d = R cam);
there is no pose regulariser.  Intrinsics and lens distortion can be stated (data/cameras.py: every camera there is central, o = t,
d = R cam, so its rays refine like the plain camera's) but are not refined.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .baked import BakedField, BrickBakedField, _check, _ray_args, _stream, check_render_args
from .baked_train import bias_corrected_rate, check_steps, check_target_shape, finite_numbers, march_flags, ray_norm


def check_ray_model(model) -> None:
    """ValueError for NDC rays: None (the plain pinhole rays) and a pinhole _lib.KnerfRayModel pass"""
    if model is not None and int(getattr(model, "ndc", 0)):
        raise ValueError("camera poses cannot be refined through NDC rays: the pose does not enter them as o = t, d = R cam "
                         "(draw the rays with ndc=False)")


def ray_gradients(field, origins, directions, near, far, target, step=None, white_background=False, termination=0.0, n_total=None,
                  lanes_per_ray=0):
    """knerf_baked_ray_gradients / knerf_baked_ray_gradients_bricks on a BakedField / BrickBakedField: (grad_origin [n,3],
    grad_direction [n,3], loss) of L = 1 / (3 N) sum (out - target)^2, the objective of BakedFieldOptimizer.accumulate marched over
    the field's occupancy bits with the same step, white_background and termination (the field is not changed).  The loss is a float64
    device scalar as accumulate returns it; n_total is the N of the loss when the batch is one part of several (default: this batch's
    rays).  lanes_per_ray: the kernel variant, as in render().  Nothing waits for the GPU."""
    import torch
    from . import _lib
    from .runtime import _f32, _ptr
    if hasattr(field, "dequantize"):
        raise ValueError("ray_gradients needs a BakedField or a BrickBakedField, got a QuantizedBrickField: dequantize() gives one")
    if not isinstance(field, (BakedField, BrickBakedField)):
        raise ValueError(f"ray_gradients needs a BakedField or a BrickBakedField, got {type(field).__name__}")
    check_render_args(step, termination, ("image",), field.sh_degree, lanes_per_ray)
    dev = field.device
    o, d, n, h, (near_t, near0), (far_t, far0) = _ray_args(field, origins, directions, near, far, step)
    tg = _f32(target, dev)
    check_target_shape(tuple(tg.shape), n)
    norm = ray_norm(n, n_total)
    go = torch.empty((n, 3), device=dev, dtype=torch.float32)
    gd = torch.empty((n, 3), device=dev, dtype=torch.float32)
    sq = torch.empty((n,), device=dev, dtype=torch.float32)
    if n:
        name = "knerf_baked_ray_gradients_bricks" if isinstance(field, BrickBakedField) else "knerf_baked_ray_gradients"
        _check(getattr(_lib.load(), name)(_stream(dev), C.byref(field._c), _ptr(o), _ptr(d), _ptr(near_t), _ptr(far_t), near0, far0, _ptr(tg),
                                          n, norm, h, float(termination), march_flags(white_background, lanes_per_ray), _ptr(go), _ptr(gd),
                                          _ptr(sq)), name)
    return go, gd, sq.to(torch.float64).sum() / (3.0 * max(norm, 1))


def pose_gradients(grad_origin, grad_direction, directions, view, n_views):
    """knerf_pose_gradients: float64 [n_views, 6] on the device, per camera the sum of grad_origin (columns 0..2, tau) and of
    directions x grad_direction (columns 3..5, omega) over its rays.  view: an integer tensor [n], the camera of every ray (int32 on
    the device is passed as it is); an index outside [0, n_views) is skipped.  Deterministic: the same inputs give the same bits."""
    import torch
    from . import _lib
    from .runtime import _f32, _ptr
    dev = grad_origin.device
    go, gd, d = (_f32(x, dev).reshape(-1, 3) for x in (grad_origin, grad_direction, directions))
    vw = view if isinstance(view, torch.Tensor) else torch.as_tensor(np.asarray(view))
    if vw.dtype.is_floating_point or vw.dtype == torch.bool:
        raise ValueError(f"view must hold integers, got {vw.dtype}")
    vw = vw.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    n = go.shape[0]
    if gd.shape[0] != n or d.shape[0] != n or vw.numel() != n:
        raise ValueError(f"{n} origin gradients for {gd.shape[0]} direction gradients, {d.shape[0]} directions and {vw.numel()} views")
    V = int(n_views)
    if V < 1:
        raise ValueError(f"n_views must be positive, got {n_views!r}")
    out = torch.empty((V, 6), device=dev, dtype=torch.float64)
    _check(_lib.load().knerf_pose_gradients(_stream(dev), _ptr(go), _ptr(gd), _ptr(d), _ptr(vw), n, V, _ptr(out)), "knerf_pose_gradients")
    return out


def rodrigues(omega):
    """exp(omega^) for a float64 tensor omega [V,3]: I + sin(th)/th K + (1 - cos th)/th^2 K^2 (the series' first terms below
    th = 1e-4, where the quotients lose their digits); float64 [V,3,3].  No host read."""
    import torch
    w = omega.to(torch.float64)
    th = torch.linalg.norm(w, dim=-1)[:, None, None]
    K = torch.zeros((w.shape[0], 3, 3), device=w.device, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2] = -w[:, 2], w[:, 1]
    K[:, 1, 0], K[:, 1, 2] = w[:, 2], -w[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -w[:, 1], w[:, 0]
    small = th < 1e-4
    safe = torch.where(small, torch.ones_like(th), th)
    a = torch.where(small, 1.0 - th * th / 6.0, torch.sin(safe) / safe)
    b = torch.where(small, 0.5 - th * th / 24.0, (1.0 - torch.cos(safe)) / (safe * safe))
    return torch.eye(3, device=w.device, dtype=torch.float64) + a * K + b * (K @ K)


def check_pose_args(c2w_shape, learning_rate_rotation, learning_rate_translation, beta_1, beta_2, epsilon):
    """ValueError unless the poses are [V,4,4] with V >= 1, both learning rates are finite and >= 0 with one of them > 0, both betas
    lie in [0, 1) and epsilon is finite and > 0; returns the five numbers as floats"""
    if len(c2w_shape) != 3 or tuple(c2w_shape[1:]) != (4, 4) or c2w_shape[0] < 1:
        raise ValueError(f"c2w must be [V,4,4] camera-to-world matrices, got {tuple(c2w_shape)}")
    lr_r, lr_t, b1, b2, eps = finite_numbers((("learning_rate_rotation", learning_rate_rotation),
                                              ("learning_rate_translation", learning_rate_translation), ("beta_1", beta_1),
                                              ("beta_2", beta_2), ("epsilon", epsilon)))
    if lr_r < 0.0 or lr_t < 0.0 or not (lr_r > 0.0 or lr_t > 0.0):
        raise ValueError(f"learning rates must be >= 0 and one of them > 0, got {learning_rate_rotation!r} and {learning_rate_translation!r}")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"beta_1 and beta_2 must lie in [0, 1), got {beta_1!r} and {beta_2!r}")
    if not eps > 0.0:
        raise ValueError(f"epsilon must be > 0, got {epsilon!r}")
    return lr_r, lr_t, b1, b2, eps


def fixed_mask(fixed_views, n_views) -> np.ndarray:
    """bool [V] from None, indices or a bool mask; ValueError on an index outside [0, V), a mask of another length, or all views fixed"""
    mask = np.zeros(int(n_views), dtype=bool)
    if fixed_views is None:
        return mask
    fv = np.asarray(fixed_views.cpu() if hasattr(fixed_views, "cpu") else fixed_views)
    if fv.dtype == bool:
        if fv.shape != mask.shape:
            raise ValueError(f"a fixed_views mask must hold {n_views} values, got {fv.shape}")
        mask = fv.copy()
    else:
        if fv.size and (fv.dtype.kind not in "iu" or fv.min() < 0 or fv.max() >= n_views):
            raise ValueError(f"fixed_views must be indices in [0, {n_views}) or a bool mask, got {fixed_views!r}")
        mask[fv.reshape(-1).astype(np.int64)] = True
    if mask.all():
        raise ValueError("every view is fixed: there is no pose to refine")
    return mask


class PoseOptimizer:
    """Adam on the rigid motion of V cameras against a baked field.  `poses` is the live [V,4,4] float32 device tensor of
    camera-to-world matrices (equal to the input bit for bit after construction); accumulate() adds the gradient of a batch, apply()
    takes one step:  Keras-form Adam on each view's 6-vector gradient (tau, omega) in the form of baked_train_apply_kernel
    (m += (g - m)(1 - beta_1), v += (g g - v)(1 - beta_2), step = rate m / (sqrt(v) + epsilon), rate the bias-corrected
    baked_train.bias_corrected_rate of learning_rate_translation resp. learning_rate_rotation), then
        R <- exp(-step_omega^) R   (Rodrigues, in float64, stored as float32),      t <- t - step_tau.
    The gradient is taken in the LEFT tangent frame at the current pose (R <- exp(omega^) R, t <- t + tau at 0) and the moments are
    kept in that frame from step to step: they are NOT transported when the pose moves.  For the small corrections this is made for
    (degrees, not turns) the frames of successive steps differ by the step itself, a second-order effect.
    fixed_views (indices or a bool mask) anchors cameras: the joint problem of field and poses is only determined up to one rigid
    motion of everything, and a fixed camera removes that freedom.  Their poses and moments never change, bit for bit.
    State: V x (12 + 6 + 6) numbers on the device; `step` counts the steps applied (the host's count, no device read)."""

    def __init__(self, c2w, learning_rate_rotation, learning_rate_translation, beta_1=0.9, beta_2=0.999, epsilon=1e-7, fixed_views=None,
                 device=None):
        import torch
        src = c2w if isinstance(c2w, torch.Tensor) else torch.as_tensor(np.asarray(c2w, dtype=np.float32))
        self.learning_rate_rotation, self.learning_rate_translation, self.beta_1, self.beta_2, self.epsilon = \
            check_pose_args(tuple(src.shape), learning_rate_rotation, learning_rate_translation, beta_1, beta_2, epsilon)
        self.n_views = int(src.shape[0])
        fixed = fixed_mask(fixed_views, self.n_views)
        dev = torch.device(device if device is not None else (src.device if src.is_cuda else "cuda"))
        self.poses = src.to(device=dev, dtype=torch.float32).clone().contiguous()
        self._fixed = torch.as_tensor(fixed).to(dev)
        self._m = torch.zeros((self.n_views, 6), device=dev, dtype=torch.float64)
        self._v = torch.zeros_like(self._m)
        self._grad = torch.zeros_like(self._m)
        self.step = 0

    @property
    def device(self):
        return self.poses.device

    @property
    def fixed_views(self):
        """bool [V] on the device"""
        return self._fixed

    def gradients(self):
        """float64 [V,6] on the device: the rigid-motion gradient accumulated since the last apply(), tau first, then omega"""
        return self._grad.clone()

    def accumulate(self, field, origins, directions, near, far, target, view, step=None, white_background=False, termination=0.0,
                   n_total=None, lanes_per_ray=0, ray_model=None):
        """field.ray_gradients on the batch, then knerf_pose_gradients with `view` (an integer tensor [n]: the camera of every ray,
        RayBatchDataset.last_view): ADDS the batch's [V,6] gradient to the accumulated one and returns the batch's loss (float64
        device scalar).  The rays must have been generated from `poses` as o = t, d = R cam; ray_model: the generator's
        knerf_ray_model if it has one -- NDC rays are refused with ValueError before any launch.  step, white_background, termination,
        n_total, lanes_per_ray: as field.ray_gradients (beside a field optimiser: that optimiser's own)."""
        check_ray_model(ray_model)
        go, gd, loss = ray_gradients(field, origins, directions, near, far, target, step=step, white_background=white_background,
                                     termination=termination, n_total=n_total, lanes_per_ray=lanes_per_ray)
        from .runtime import _f32
        self._grad += pose_gradients(go, gd, _f32(directions, field.device).reshape(-1, 3), view, self.n_views)
        return loss

    def apply(self):
        """one Adam step from the accumulated gradient on every view that is not fixed; the gradient is zeroed"""
        import torch
        t = self.step + 1
        move = ~self._fixed[:, None]
        g = self._grad
        m = self._m + (g - self._m) * (1.0 - self.beta_1)
        v = self._v + (g * g - self._v) * (1.0 - self.beta_2)
        rate_t = bias_corrected_rate(self.learning_rate_translation, self.beta_1, self.beta_2, t)      # host doubles: no copy, no wait
        rate_r = bias_corrected_rate(self.learning_rate_rotation, self.beta_1, self.beta_2, t)
        unit = m / (torch.sqrt(v) + self.epsilon)
        delta = torch.where(move, torch.cat([unit[:, :3] * rate_t, unit[:, 3:] * rate_r], dim=1), torch.zeros_like(m))
        self._m, self._v = torch.where(move, m, self._m), torch.where(move, v, self._v)
        rot = (rodrigues(-delta[:, 3:]) @ self.poses[:, :3, :3].to(torch.float64)).to(torch.float32)
        tr = (self.poses[:, :3, 3].to(torch.float64) - delta[:, :3]).to(torch.float32)
        self.poses[:, :3, :3] = torch.where(move[:, :, None], rot, self.poses[:, :3, :3])         # in place: `poses` stays the live tensor
        self.poses[:, :3, 3] = torch.where(move, tr, self.poses[:, :3, 3])
        self._grad.zero_()
        self.step = t

    def state_dict(self):
        """{"poses", "m", "v", "fixed", "step"}: host copies (NumPy) of the state, enough to go on where this optimiser stands"""
        return {"poses": self.poses.cpu().numpy(), "m": self._m.cpu().numpy(), "v": self._v.cpu().numpy(),
                "fixed": self._fixed.cpu().numpy(), "step": int(self.step)}

    def load_state_dict(self, state):
        """the state state_dict() returned; ValueError on a missing key or another number of views.  The accumulated gradient is zeroed."""
        import torch
        missing = [k for k in ("poses", "m", "v", "fixed", "step") if k not in state]
        if missing:
            raise ValueError(f"not a PoseOptimizer state (missing {missing})")
        poses, m, v, fixed = (np.asarray(state[k]) for k in ("poses", "m", "v", "fixed"))
        V = self.n_views
        if poses.shape != (V, 4, 4) or m.shape != (V, 6) or v.shape != (V, 6) or fixed.shape != (V,) or int(state["step"]) < 0:
            raise ValueError(f"the state holds poses {poses.shape}, moments {m.shape} / {v.shape}, fixed {fixed.shape}; this optimiser has {V} views")
        self.poses.copy_(torch.as_tensor(poses.astype(np.float32)))
        self._m.copy_(torch.as_tensor(m.astype(np.float64)))
        self._v.copy_(torch.as_tensor(v.astype(np.float64)))
        self._fixed.copy_(torch.as_tensor(fixed.astype(bool)))
        self._grad.zero_()
        self.step = int(state["step"])


def pose_errors(c2w, truth):
    """(rotation error in degrees [V], translation error [V]) of poses against the true ones, float64 NumPy: the angle of R R_true^T,
    taken from |R R_true^T - I|_F = 2 sqrt(2) sin(angle / 2) (the arc cosine of the trace loses half its digits near 0), and
    |t - t_true|"""
    a = np.asarray(c2w.cpu() if hasattr(c2w, "cpu") else c2w, dtype=np.float64)
    b = np.asarray(truth.cpu() if hasattr(truth, "cpu") else truth, dtype=np.float64)
    rel = a[:, :3, :3] @ np.transpose(b[:, :3, :3], (0, 2, 1))
    chord = np.linalg.norm(rel - np.eye(3), axis=(1, 2)) / (2.0 * np.sqrt(2.0))
    return np.degrees(2.0 * np.arcsin(np.clip(chord, 0.0, 1.0))), np.linalg.norm(a[:, :3, 3] - b[:, :3, 3], axis=1)


def fit_with_poses(opt, pose_opt, batches, near, far, steps=None, field_steps_first=0, field=None, **march):
    """Field and poses together.  `batches` is a RayBatchDataset (or anything with its set_cameras() / last_view pair and, optionally,
    ray_model()): it is told to draw every batch with pose_opt.poses as they stand, and per step the SAME batch goes through
    opt.accumulate and pose_opt.accumulate (both gradients at the same field and poses), then opt.apply() and pose_opt.apply().
    opt: a BakedFieldOptimizer or BrickFieldOptimizer, whose live field and march settings the pose gradient uses; None: poses only,
    against `field` (a BakedField or BrickBakedField, frozen) marched with **march (step, white_background, termination,
    lanes_per_ray as field.ray_gradients takes them).  field_steps_first: that many first steps move the field alone, so that it
    settles before the cameras do.  steps: at most that many batches (None: all of them).
    An optimiser built with loss= / regularizers= uses that objective for the FIELD step only: the pose gradient (ray_gradients) stays
    that of the mean squared error.
    Returns {"loss": [...]} (the data term before each step), read from the device once, after the last step.  NDC rays (batches
    whose ray_model() says so) raise ValueError before the first launch.  The dataset keeps the provider afterwards: its next batches
    are drawn with the refined poses (set_cameras(None) gives the stored ones back)."""
    import torch
    check_steps(steps)
    check_steps(field_steps_first, "field_steps_first", optional=False)
    if not isinstance(pose_opt, PoseOptimizer):
        raise ValueError(f"pose_opt must be a PoseOptimizer, got {type(pose_opt).__name__}")
    if (opt is None) == (field is None):
        raise ValueError("give either a field optimiser (opt) or, with opt=None, the frozen field= to refine the poses against")
    if opt is not None and march:
        raise ValueError(f"with a field optimiser the march is the optimiser's own; got {sorted(march)}")
    if opt is None and field_steps_first:
        raise ValueError("field_steps_first needs a field optimiser")
    if not (hasattr(batches, "set_cameras") and hasattr(batches, "last_view")):
        raise ValueError("batches must draw its rays from the current poses: a RayBatchDataset (set_cameras / last_view)")
    model = batches.ray_model() if hasattr(batches, "ray_model") else None
    check_ray_model(model)
    if opt is not None:
        field = opt.field
        march = dict(step=opt.step, white_background=opt.white_background, termination=opt.termination, lanes_per_ray=opt.lanes_per_ray)
    batches.set_cameras(lambda: pose_opt.poses)
    losses = []
    for k, (target, (o, d, _t)) in enumerate(batches):
        if steps is not None and k >= int(steps):
            break
        moving = k >= int(field_steps_first)
        if opt is not None:
            z, c = getattr(batches, "last_depth", None) or (None, None)       # the field's depth term; the pose gradient stays MSE
            losses.append(opt.accumulate(o, d, near, far, target, depth=z, depth_weight=c))
            if moving:
                pose_opt.accumulate(field, o, d, near, far, target, batches.last_view, ray_model=model, **march)
            if getattr(opt, "regularized", False):
                opt.last_regularizer = opt.regularize()
            opt.apply()
        else:
            losses.append(pose_opt.accumulate(field, o, d, near, far, target, batches.last_view, ray_model=model, **march))
        if moving:
            pose_opt.apply()
    return {"loss": torch.stack(losses).cpu().tolist() if losses else []}
