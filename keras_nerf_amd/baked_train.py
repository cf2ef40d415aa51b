"""Optimising a baked field against ray batches (extension, no reference counterpart; PlenOctrees and Plenoxels optimise their grids
against the photographs after conversion in this way).

The arithmetic is HIP (csrc/baked_train.hip: knerf_baked_train_rays marches a batch, evaluates the squared error and scatters its
gradient into the lattice; knerf_baked_train_apply is Adam and rewrites the records; csrc/baked_grow.hip: knerf_baked_train_tv, the
optional total-variation regulariser between the two, and the resampling behind fit_coarse_to_fine; include/knerf.h holds the contract).  torch is
used for device memory, streams and the index plumbing of the construction only.  No step waits for the GPU.
With loss= / regularizers= (the objective of NeRF.compile: keras_nerf_amd/losses.py) the gradient launch is knerf_baked_train_rays_ext,
the same march under a robust loss and the distortion / opacity-entropy regularisers of a ray's weights.
With background= / opacity_loss= and [n,4] targets (rgb and the photograph's alpha) it is knerf_baked_train_rays_rgba: prediction and
photograph composited over a background per ray, and a loss between the ray's opacity and the alpha.

What keeps skipping empty cells exact while the numbers move:
  support    the field's occupancy bits at the start, grown by `dilation` cells, fixed for the optimiser's lifetime: the bits of every
             march, of the live field's renders included;
  slots      the lattice points that are a corner of a support cell; master values, gradients and both Adam moments are rows
             [n_slots][1 + 3 K] fp32 (sigma, then [k][c]); nothing but the int32 slot table is dense over the lattice;
  sigma      is trainable only at slots whose 8 adjacent cells all lie in the support (or outside the lattice) and is projected to >= 0:
             every other point has sigma = 0 and keeps it, so a cell outside the support has sigma = 0 at all 8 corners for ever.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .baked import (BakedField, _check, _ray_args, _stream, _unpack_words, check_depth_loss, check_render_args, check_threshold, n_coefficients,
                    takes_depth_loss)


def is_number(v, finite_as=float, integer=False) -> bool:
    """whether v is a number and no bool: an int, a float or their NumPy kinds that is finite as a `finite_as` (float, or np.float32
    where the value ends up in one); with integer=True an int or a NumPy integer"""
    if integer:
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    return not isinstance(v, bool) and isinstance(v, (int, float, np.floating, np.integer)) and bool(np.isfinite(finite_as(v)))


def finite_numbers(named, finite_as=float):
    """the values of `named` ((name, value) pairs) as floats; ValueError for the first that is not is_number(value, finite_as)"""
    for name, v in named:
        if not is_number(v, finite_as):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    return tuple(float(v) for _, v in named)


def check_optimizer_args(learning_rate_sigma, learning_rate_sh, beta_1, beta_2, epsilon, dilation):
    """ValueError unless both learning rates and epsilon are finite and > 0, both betas lie in [0, 1) and dilation is an integer 0..8
    (what knerf_occupancy_from_grid takes); returns them as (float, float, float, float, float, int)"""
    lrs, lrc, b1, b2, eps = finite_numbers((("learning_rate_sigma", learning_rate_sigma), ("learning_rate_sh", learning_rate_sh),
                                            ("beta_1", beta_1), ("beta_2", beta_2), ("epsilon", epsilon)))
    if not (lrs > 0.0 and lrc > 0.0):
        raise ValueError(f"learning rates must be > 0, got {learning_rate_sigma!r} and {learning_rate_sh!r}")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"beta_1 and beta_2 must lie in [0, 1), got {beta_1!r} and {beta_2!r}")
    if not np.float32(eps) > 0.0:
        raise ValueError(f"epsilon must be > 0 (as a float32), got {epsilon!r}")
    if not is_number(dilation, integer=True) or not 0 <= int(dilation) <= 8:
        raise ValueError(f"dilation must be an integer 0..8, got {dilation!r}")
    return lrs, lrc, b1, b2, eps, int(dilation)


def check_tv_args(tv_sigma, tv_sh, tv_epsilon):
    """ValueError unless both total-variation weights are finite and >= 0 and tv_epsilon is finite and > 0 (as a float32); returns
    them as floats"""
    out = finite_numbers((("tv_sigma", tv_sigma), ("tv_sh", tv_sh), ("tv_epsilon", tv_epsilon)), np.float32)
    if out[0] < 0.0 or out[1] < 0.0:
        raise ValueError(f"tv_sigma and tv_sh must be >= 0, got {tv_sigma!r} and {tv_sh!r}")
    if not np.float32(out[2]) > 0.0:
        raise ValueError(f"tv_epsilon must be > 0 (as a float32), got {tv_epsilon!r}")
    return out


def check_steps(steps, name="steps", optional=True) -> None:
    """ValueError unless `steps` is a non-negative integer, or None where that is allowed (fit: every batch)"""
    if (steps is None and not optional) or (steps is not None and (isinstance(steps, bool) or int(steps) != steps or int(steps) < 0)):
        raise ValueError(f"{name} must be a non-negative integer{' or None' if optional else ''}, got {steps!r}")


def ray_norm(n, n_total) -> int:
    """the N of a launch's loss: n_total, or the batch's n rays; ValueError for an n_total below 1 beside rays"""
    norm = n if n_total is None else int(n_total)
    if norm < 1 and n:
        raise ValueError(f"n_total must be a positive ray count, got {n_total!r}")
    return norm


def march_flags(white_background, lanes_per_ray) -> int:
    """the flag word of a training march (include/knerf.h): the background, empty cells skipped, the kernel variant"""
    from . import _lib
    return (_lib.BAKED_WHITE_BACKGROUND if white_background else 0) | _lib.BAKED_SKIP_EMPTY | (int(lanes_per_ray) << _lib.BAKED_LANES_SHIFT)


def slot_masks(occ, res):
    """(touched, free), bool [Rx,Ry,Rz] on occ's device, from the support cells occ [Rx-1,Ry-1,Rz-1]: the lattice points that are a
    corner of a support cell (the slots), and those none of whose 8 adjacent cells is a lattice cell outside the support (where sigma
    is trainable)"""
    import torch
    cx, cy, cz = occ.shape
    touched = torch.zeros(res, device=occ.device, dtype=torch.bool)
    free = torch.ones(res, device=occ.device, dtype=torch.bool)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                touched[a:a + cx, b:b + cy, c:c + cz] |= occ
                free[a:a + cx, b:b + cy, c:c + cz] &= occ
    return touched, free


def check_target_shape(shape, n_rays) -> None:
    """ValueError unless a target of this shape is [n_rays, 3]"""
    if len(shape) != 2 or shape[1] != 3 or shape[0] != n_rays:
        raise ValueError(f"target must be [{n_rays}, 3], one colour per ray; got {tuple(shape)}")


def check_objective(loss, regularizers):
    """The knerf_objective record of a grid optimiser's `loss=` / `regularizers=` keywords (losses.objective_from: every spelling
    NeRF.compile takes), or None for the plain objective (mean squared error, both weights 0): the optimiser then calls the plain entry
    point.  ValueError, before any device work, for what losses refuses and for a RayRegularizers whose nets is not the default: a grid
    has no coarse / fine pair."""
    from . import losses
    r = losses.regularizers_from(regularizers)
    if r.nets != "both":
        raise ValueError(f"RayRegularizers nets={r.nets!r}: a baked field has no coarse / fine pair, leave nets at its default")
    obj = losses.objective_from(loss, r)
    return None if losses.is_plain(obj) else obj


TERM_NAMES = ("photometric", "mse", "distortion", "opacity_entropy")


def term_means(total, norm):
    """{name: mean} from the summed columns `total` [4], [5] or [6] of a launch's per-ray terms: photometric and mse are means over rays
    and channels, distortion, opacity_entropy, (the fifth column) opacity and (the sixth) depth over rays (N = norm)"""
    n = float(max(norm, 1))
    means = {"photometric": total[0] / (3.0 * n), "mse": total[1] / (3.0 * n)}
    for i, name in enumerate((TERM_NAMES + ("opacity", "depth"))[2:total.shape[0]], 2):
        means[name] = total[i] / n
    return means


def objective_value(obj, terms, norm):
    """(loss, {name: mean}) from the per-ray terms [n, 4] of an extended launch, float64 device scalars: the terms are summed in float64
    on the device (term_means; N = norm); loss = photometric + distortion weight x mean D + opacity_entropy weight x mean H, the
    function whose gradient the launch added."""
    import torch
    means = term_means(terms.to(torch.float64).sum(dim=0), norm)
    loss = means["photometric"] + float(obj.distortion) * means["distortion"] + float(obj.opacity_entropy) * means["opacity_entropy"]
    return loss, means


def fit_terms(out, rows):
    """adds the four lists of TERM_NAMES (with "opacity" behind them where the steps were rgba launches, and "depth" where they were
    depth launches) to a fit() dict from the per-step objective_terms() (one device read)"""
    import torch
    names = TERM_NAMES + tuple(k for k in ("opacity", "depth") if rows and all(k in r for r in rows))
    both = torch.stack([torch.stack([r[k] for k in names]) for r in rows]).cpu() if rows else torch.zeros((0, 4))
    for i, k in enumerate(names):
        out[k] = both[:, i].tolist()
    return out


BACKGROUNDS = ("black", "white", "random")


class RgbaTargets:
    """The keywords background=, opacity_loss=, target_background= and background_seed= of a grid optimiser, checked
    on the host, and what an accumulate() makes of them: the knerf_baked_rgba record of a launch, or None where the launch is the one
    the optimiser made before these keywords existed.
      white          the launch's white-background flag: white_background=True or background="white"
      mode           None (the flag's colour), "random" (torch.rand per launch) or "colour" (`colour` on every ray)
      opacity        lambda_o, the weight of mean (O - alpha)^2
      stored         0.0 or 1.0: what the targets' rgb is composited over (target_background; default: the flag)"""

    def __init__(self, white_background=False, background=None, opacity_loss=0.0, target_background=None, background_seed=0):
        from .baked import check_colour
        white = bool(white_background)
        self.mode, self.colour = None, None
        if background is None or (isinstance(background, str) and background == "white"):
            white = white or background == "white"
        elif isinstance(background, str):
            if background not in BACKGROUNDS:
                raise ValueError(f"background must be None, one of {BACKGROUNDS} or a colour (r, g, b), got {background!r}")
            if white:
                raise ValueError(f"white_background=True contradicts background={background!r}")
            self.mode = "random" if background == "random" else None
        else:
            self.colour = check_colour(background)
            if white:
                raise ValueError(f"white_background=True contradicts background={background!r}")
            self.mode = "colour"
        self.white = white
        if not is_number(opacity_loss, np.float32) or float(opacity_loss) < 0.0:
            raise ValueError(f"opacity_loss must be a finite number >= 0, got {opacity_loss!r}")
        self.opacity = float(opacity_loss)
        if target_background not in (None, "black", "white"):
            raise ValueError(f'target_background must be None, "black" or "white", got {target_background!r}')
        self.stored = float(white) if target_background is None else float(target_background == "white")
        if not is_number(background_seed, integer=True):
            raise ValueError(f"background_seed must be an integer, got {background_seed!r}")
        self.seed = int(background_seed)
        self._generator = None
        self.last_background = None

    def split_target(self, tg, n):
        """(rgb [n,3], alpha [n] | None) of a float32 target [n,3] or [n,4]; ValueError for another shape"""
        if tg.dim() == 2 and tg.shape[1] == 4 and tg.shape[0] == n:
            return tg[:, :3].contiguous(), tg[:, 3].contiguous()
        if tg.dim() != 2 or tg.shape[1] != 3 or tg.shape[0] != n:
            raise ValueError(f"target must be [{n}, 3] or [{n}, 4] (rgb, or rgb and alpha, per ray); got {tuple(tg.shape)}")
        return tg, None

    def record(self, alpha, n, device, background=None):
        """The knerf_baked_rgba of one launch, or None: no alpha, no background but the flag's and no opacity loss.  `background`: the
        per-call [n,3] override of accumulate().  The tensors the record points to are kept in last_background and on the record."""
        import torch
        from . import _lib
        from .runtime import _ptr
        bg = None
        if background is not None:
            if isinstance(background, torch.Tensor):
                bg = background.to(device=device, dtype=torch.float32).contiguous()
            else:
                bg = torch.as_tensor(np.asarray(background, dtype=np.float32)).to(device).contiguous()
            if tuple(bg.shape) != (n, 3) or not bool(((bg >= 0) & (bg <= 1)).all()):      # (a NaN fails both comparisons)
                raise ValueError(f"background must be [{n}, 3] with finite values in [0, 1], got shape {tuple(bg.shape)}")
        elif self.mode == "random":
            if alpha is None:
                raise ValueError('background="random" needs [n, 4] targets: a random background against an RGB-only target is wrong')
            if self._generator is None:
                self._generator = torch.Generator(device=device)
                self._generator.manual_seed(self.seed)
            bg = torch.rand((n, 3), device=device, dtype=torch.float32, generator=self._generator)
        elif self.mode == "colour":
            bg = torch.tensor(self.colour, device=device, dtype=torch.float32).expand(n, 3).contiguous()
        if self.opacity > 0.0 and alpha is None:
            raise ValueError("opacity_loss > 0 needs [n, 4] targets: the fourth column is the alpha the opacity is compared with")
        self.last_background = bg
        if bg is None and alpha is None and self.opacity == 0.0:
            return None
        rec = _lib.KnerfBakedRgba(_ptr(bg), _ptr(alpha), self.stored, self.opacity)
        rec._keep = (bg, alpha)
        return rec


def rgba_value(obj, rec, terms, norm):
    """objective_value for the per-ray terms [n, 5] of an rgba launch: the fifth mean is "opacity", the unweighted mean of
    (O - alpha)^2, and the loss adds the record's weight times it.  obj None: the plain objective (mean squared error)."""
    import torch
    means = term_means(terms.to(torch.float64).sum(dim=0), norm)
    loss = means["photometric"] + float(rec.opacity) * means["opacity"]
    if obj is not None:
        loss = loss + float(obj.distortion) * means["distortion"] + float(obj.opacity_entropy) * means["opacity_entropy"]
    return loss, means


def depth_record(depth_loss, depth, depth_weight, n, device):
    """The knerf_baked_depth of one launch, or None: depth_loss is 0 (depth tensors are then ignored: the launch is the one made
    without them).  depth [n]: the rays' depth targets in ray-parameter units; depth_weight [n] >= 0 or None (every ray 1).  ValueError
    for depth_loss > 0 without depth and for another shape.  The tensors the record points to are kept on it."""
    from . import _lib
    from .runtime import _f32, _ptr
    if depth_loss == 0.0:
        return None
    if depth is None:
        raise ValueError("depth_loss > 0 needs depth: one depth target per ray, in ray-parameter units")
    z = _f32(depth, device)
    c = None if depth_weight is None else _f32(depth_weight, device)
    for name, t in (("depth", z), ("depth_weight", c)):
        if t is not None and tuple(t.shape) != (n,):
            raise ValueError(f"{name} must be [{n}], one value per ray; got {tuple(t.shape)}")
    rec = _lib.KnerfBakedDepth(_ptr(z), _ptr(c), depth_loss)
    rec._keep = (z, c)
    return rec


def depth_value(obj, rgba, rec, terms, norm):
    """objective_value for the per-ray terms [n, 6] of a depth launch: the sixth mean is "depth", the unweighted mean of c (Z - z*)^2,
    and the loss adds the record's weight times it.  obj None: the plain objective; rgba None: no opacity loss."""
    import torch
    means = term_means(terms.to(torch.float64).sum(dim=0), norm)
    loss = means["photometric"] + float(rec.depth) * means["depth"]
    if rgba is not None:
        loss = loss + float(rgba.opacity) * means["opacity"]
    if obj is not None:
        loss = loss + float(obj.distortion) * means["distortion"] + float(obj.opacity_entropy) * means["opacity_entropy"]
    return loss, means


def bias_corrected_rate(learning_rate: float, beta_1: float, beta_2: float, t: int) -> float:
    """Keras-form Adam: learning_rate sqrt(1 - beta_2^t) / (1 - beta_1^t) in double, t the step being applied (from 1)"""
    return float(learning_rate) * float(np.sqrt(1.0 - float(beta_2) ** t)) / (1.0 - float(beta_1) ** t)


class GridOptimizer:
    """What the optimisers of a baked field share, whatever its storage (BakedFieldOptimizer here, BrickFieldOptimizer in
    baked_bricks_train.py): the keywords' checks, the gradient launch, Adam's launch, train_step() and fit().  A subclass names its
    entry points and builds its state:
      _train_rays            the stem of its gradient launch; accumulate() appends "", "_ext", "_rgba" or "_depth"
      _check_source(source)  its refusal of a source of the wrong kind
      _check_lanes(sh_degree, lanes_per_ray)   the lane counts its gradient kernel is built for
      _build(source)         the live `field`, `_master` [rows][1 + 3 K] fp32, `n_slots` and its own index tensors
      _state()               its struct for the launches, over `field` and `_grad`
      _apply_launch()        (the name of its Adam launch, the arguments between the struct and the master rows)"""

    _rgba = RgbaTargets()               # the rgba keywords at their defaults: every launch is what it was without them
    _train_rays = None
    depth_loss = 0.0                    # lambda_z at its default: no launch is a depth launch

    @takes_depth_loss
    def __init__(self, source, learning_rate_sigma, learning_rate_sh, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dilation=0, step=None,
                 white_background=False, termination=0.0, lanes_per_ray=0, loss=None, regularizers=None, background=None,
                 opacity_loss=0.0, target_background=None, background_seed=0):
        """every keyword is checked (ValueError) before `source` is touched and before the library is loaded"""
        import torch
        self._rgba = RgbaTargets(white_background, background, opacity_loss, target_background, background_seed)
        self.learning_rate_sigma, self.learning_rate_sh, self.beta_1, self.beta_2, self.epsilon, self.dilation = \
            check_optimizer_args(learning_rate_sigma, learning_rate_sh, beta_1, beta_2, epsilon, dilation)
        self.objective = check_objective(loss, regularizers)               # None: the plain objective, the plain entry point
        self._terms = None                                                  # the last accumulate's means (objective_terms)
        self._check_source(source)
        check_render_args(step, termination, ("image",))
        self.lanes_per_ray = self._check_lanes(source.sh_degree, lanes_per_ray)
        self.step, self.white_background, self.termination = step, self._rgba.white, float(termination)
        self._width = 1 + 3 * n_coefficients(source.sh_degree)
        self._build(source)
        self._grad = torch.zeros_like(self._master)
        self._m, self._v = torch.zeros_like(self._master), torch.zeros_like(self._master)
        self.iterations = 0                                                 # steps applied; the host's count, no device read
        self._c = self._state()

    def _check_source(self, source) -> None:
        pass

    # ---- the two launches
    def accumulate(self, origins, directions, near, far, target, n_total=None, background=None, depth=None, depth_weight=None):
        """knerf_baked_train_rays / knerf_baked_bricks_train_rays: adds the gradient of the batch's mean squared error to the gradient
        rows and returns the loss, a float64 device scalar (the per-ray errors are summed in float64 on the device; nothing waits).
        n_total: the N of the loss 1 / (3 N) sum (out - target)^2 when the batch is one part of several accumulated before apply()
        (default: this batch's rays).
        With a loss= / regularizers= objective that is not the plain one: knerf_baked_train_rays_ext /
        knerf_baked_bricks_train_rays_ext, and the value returned is that of the function whose gradient was added, the mean of rho
        plus distortion x mean D plus opacity_entropy x mean H (the per-ray terms summed in float64 on the device);
        objective_terms() then gives the four means.
        With the rgba keywords (background=, opacity_loss=), an [n,4] target (the fourth column is the photograph's alpha) or a
        per-call `background` ([n,3], values in [0,1], overrides the keyword): knerf_baked_train_rays_rgba /
        knerf_baked_bricks_train_rays_rgba, the prediction and the photograph composited over the ray's own background and
        opacity_loss x mean (O - alpha)^2 added; objective_terms() then has a fifth mean, "opacity", and last_background is the
        background tensor of the launch.
        With depth_loss > 0: knerf_baked_train_rays_depth / knerf_baked_bricks_train_rays_depth, and depth_loss x the
        mean over the rays of c (Z - z*)^2 added: Z the ray's expected depth (what render() writes as depth), z* = depth [n] in
        ray-parameter units, c = depth_weight [n] >= 0 (None: 1; a ray of weight 0 has no depth term whatever its z*);
        objective_terms() then has a sixth mean, "depth".  ValueError without `depth`.  With depth_loss == 0 both are ignored."""
        import torch
        from . import _lib
        from .runtime import _f32, _ptr
        f = self.field
        o, d, n, h, (near_t, near0), (far_t, far0) = _ray_args(f, origins, directions, near, far, self.step)
        tg, alpha = self._rgba.split_target(_f32(target, f.device), n)
        rgba = self._rgba.record(alpha, n, f.device, background)
        zrec = depth_record(self.depth_loss, depth, depth_weight, n, f.device)
        norm = ray_norm(n, n_total)
        sq = torch.empty((n,), device=f.device, dtype=torch.float32)
        route = "_rgba" if rgba is not None else "_ext" if self.objective is not None else ""
        if zrec is not None:
            route = "_depth"
        args = [_stream(f.device), C.byref(self._c), _ptr(o), _ptr(d), _ptr(near_t), _ptr(far_t), near0, far0, _ptr(tg), n, norm, h,
                self.termination, march_flags(self.white_background, self.lanes_per_ray), _ptr(sq)]
        if route:
            terms = torch.zeros((n, 6 if zrec is not None else 5 if rgba is not None else 4), device=f.device, dtype=torch.float32)
            args += [C.byref(self.objective) if self.objective is not None else None, _ptr(terms)]
            if rgba is not None or zrec is not None:
                args.append(C.byref(rgba) if rgba is not None else None)
            if zrec is not None:
                args.append(C.byref(zrec))
        if n:
            _check(getattr(_lib.load(), self._train_rays + route)(*args), self._train_rays + route)
        if not route:
            return sq.to(torch.float64).sum() / (3.0 * max(norm, 1))
        if zrec is not None:
            loss, self._terms = depth_value(self.objective, rgba, zrec, terms, norm)
        elif rgba is not None:
            loss, self._terms = rgba_value(self.objective, rgba, terms, norm)
        else:
            loss, self._terms = objective_value(self.objective, terms, norm)
        return loss

    def objective_terms(self):
        """{"photometric", "mse", "distortion", "opacity_entropy"}: the four means of the last accumulate() as float64 device scalars
        (photometric: the mean of rho over rays and channels; mse: of the squared difference; the other two: mean D and mean H over
        the rays, unweighted); after an rgba launch also "opacity", the mean of (O - alpha)^2 over the rays, unweighted; after a depth
        launch "opacity" and "depth", the mean of c (Z - z*)^2 over the rays, unweighted.  None before any accumulate(), and always
        under the plain objective without the rgba and depth keywords."""
        return None if self._terms is None else dict(self._terms)

    @property
    def last_background(self):
        """the background tensor [n,3] of the last accumulate() (None: the launch used the flag's colour)"""
        return self._rgba.last_background

    def apply(self):
        """knerf_baked_train_apply / knerf_baked_bricks_train_apply: one Adam step from the accumulated gradient, the slots' records
        rewritten, their gradient zeroed"""
        from . import _lib
        from .runtime import _ptr
        t = self.iterations + 1
        name, middle = self._apply_launch()
        _check(getattr(_lib.load(), name)(
            _stream(self.field.device), C.byref(self._c), *middle, _ptr(self._master), _ptr(self._m), _ptr(self._v),
            bias_corrected_rate(self.learning_rate_sigma, self.beta_1, self.beta_2, t),
            bias_corrected_rate(self.learning_rate_sh, self.beta_1, self.beta_2, t), self.beta_1, self.beta_2, self.epsilon), name)
        self.iterations = t

    def train_step(self, origins, directions, near, far, target, depth=None, depth_weight=None):
        """accumulate, regularize (only where the class has the total-variation regulariser and a weight is > 0; its return value is
        kept in last_regularizer), apply; returns the batch's loss before the step (float64 device scalar, the data term alone).
        depth, depth_weight: the rays' depth targets and weights, as accumulate() takes them"""
        loss = self.accumulate(origins, directions, near, far, target, depth=depth, depth_weight=depth_weight)
        if getattr(self, "regularized", False):
            self.last_regularizer = self.regularize()
        self.apply()
        return loss

    def fit(self, batches, near, far, steps=None):
        """train_step on every batch of `batches` (each (target [n,3], (origins, directions, t)) as RayBatchDataset yields them; t is
        not used: the baked march places its own samples), at most `steps` of them.  {"loss": [...]}: read from the device once, after
        the last step.  With a total-variation weight > 0 the dict also holds "tv_sigma" and "tv_sh": regularize()'s two means per
        step; with an objective that is not the plain one also "photometric", "mse", "distortion" and "opacity_entropy":
        objective_terms() per step, "opacity" behind them where the steps were rgba launches and "depth" where they were depth
        launches.  Where `batches` has a `last_depth` (RayBatchDataset.set_depth: (z [n], c [n] | None) of the batch just drawn) it
        is read after each batch is drawn and passed on as the step's depth targets and weights."""
        import torch
        check_steps(steps)
        regularized = getattr(self, "regularized", False)
        losses, tvs, terms = [], [], []
        for k, (target, (o, d, _t)) in enumerate(batches):
            if steps is not None and k >= int(steps):
                break
            z, c = getattr(batches, "last_depth", None) or (None, None)
            losses.append(self.train_step(o, d, near, far, target, depth=z, depth_weight=c))
            if regularized:
                tvs.append(torch.stack(self.last_regularizer))
            if self._terms is not None:
                terms.append(self.objective_terms())
        out = {"loss": torch.stack(losses).cpu().tolist() if losses else []}
        if regularized:
            both = torch.stack(tvs).cpu() if tvs else torch.zeros((0, 2))
            out["tv_sigma"], out["tv_sh"] = both[:, 0].tolist(), both[:, 1].tolist()
        if self.objective is not None or terms:
            fit_terms(out, terms)
        return out


class TotalVariation:
    """The total-variation regulariser of a grid optimiser, for the classes that have one (BakedFieldOptimizer,
    baked_bricks_grow.BrickGridTrainer; mixed in before the optimiser class).  The class supplies _tv_launch(): (the name of its
    launch, the arguments between the struct and the weights, the rows of the per-row output)."""

    def _set_tv(self, tv_sigma, tv_sh, tv_epsilon) -> None:
        self.tv_sigma, self.tv_sh, self.tv_epsilon = check_tv_args(tv_sigma, tv_sh, tv_epsilon)
        self.last_regularizer = None                                        # what the latest train_step's regularize() returned

    @property
    def regularized(self) -> bool:
        """whether a total-variation weight is > 0: train_step then runs regularize() between accumulate() and apply()"""
        return self.tv_sigma > 0.0 or self.tv_sh > 0.0

    def tv_weights(self):
        """the weights per term knerf_baked_train_tv / knerf_baked_bricks_train_tv takes, formed in double: tv_sigma / n_slots and
        tv_sh / (3 K n_slots)"""
        return self.tv_sigma / float(self.n_slots), self.tv_sh / (float(self._width - 1) * float(self.n_slots))

    def regularize(self):
        """knerf_baked_train_tv / knerf_baked_bricks_train_tv, one launch: adds the gradient of R = tv_sigma mean_p tv_sigma(p) +
        tv_sh mean_{p,q} tv_q(p) (the total variation of the master values over the slots, include/knerf.h) to the gradient rows and
        returns the two means, unweighted, as float64 device scalars (the per-row terms are summed in float64 on the device; a brick
        record that is no slot holds (0, 0); nothing waits)."""
        import torch
        from . import _lib
        from .runtime import _ptr
        dev = self.field.device
        name, middle, rows = self._tv_launch()
        tv = torch.empty((rows, 2), device=dev, dtype=torch.float32)
        ws, wc = self.tv_weights()
        _check(getattr(_lib.load(), name)(_stream(dev), C.byref(self._c), *middle, ws, wc, self.tv_epsilon, _ptr(tv)), name)
        total = tv.to(torch.float64).sum(dim=0)
        return total[0] / float(self.n_slots), total[1] / (float(self._width - 1) * float(self.n_slots))


class BakedFieldOptimizer(TotalVariation, GridOptimizer):
    """Adam on the records of a baked field (BakedField.optimizer builds one).  `field` is the live field: it owns the records the
    optimiser rewrites, its bits are the support, and it can be rendered at any time."""

    _train_rays = "knerf_baked_train_rays"

    @takes_depth_loss
    def __init__(self, source, learning_rate_sigma, learning_rate_sh, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dilation=0, step=None,
                 white_background=False, termination=0.0, lanes_per_ray=0, tv_sigma=0.0, tv_sh=0.0, tv_epsilon=1e-6, loss=None,
                 regularizers=None, background=None, opacity_loss=0.0, target_background=None, background_seed=0):
        self._set_tv(tv_sigma, tv_sh, tv_epsilon)
        super().__init__(source, learning_rate_sigma=learning_rate_sigma, learning_rate_sh=learning_rate_sh, beta_1=beta_1, beta_2=beta_2,
                         epsilon=epsilon, dilation=dilation, step=step, white_background=white_background, termination=termination,
                         lanes_per_ray=lanes_per_ray, loss=loss, regularizers=regularizers, background=background,
                         opacity_loss=opacity_loss, target_background=target_background, background_seed=background_seed)

    @staticmethod
    def _check_lanes(sh_degree, lanes_per_ray) -> int:
        check_render_args(None, 0.0, ("image",), sh_degree, lanes_per_ray)
        return int(lanes_per_ray)

    def _build(self, source) -> None:
        import torch
        from .runtime import occupancy_words_from_grid
        dev, res, deg = source.device, source.resolution, source.sh_degree
        K = n_coefficients(deg)
        sigma = source.sigma
        support = occupancy_words_from_grid(sigma, 0.0, self.dilation, what="BakedField.optimizer")
        self.field = BakedField(source._records.clone(), support, res, source.bounds, deg, source.sigma_threshold)
        touched, free = slot_masks(_unpack_words(support, tuple(r - 1 for r in res)), res)
        index = touched.reshape(-1).nonzero().reshape(-1)                   # int64, ascending: the lattice point of every slot
        self.n_slots = int(index.numel())                                   # the one host read of the construction
        if self.n_slots == 0:
            raise ValueError("the field has no occupied cell: there is nothing to optimise")
        self._index = index
        self._point_of = index.to(torch.int32)
        self._slot_of = torch.full((touched.numel(),), -1, device=dev, dtype=torch.int32)
        self._slot_of[index] = torch.arange(self.n_slots, device=dev, dtype=torch.int32)
        self._trainable = free.reshape(-1)[index].to(torch.uint8).contiguous()
        co = source.coefficients.reshape(-1, 3 * K)[index].to(torch.float32)
        sg = sigma.reshape(-1)[index] * self._trainable.to(torch.float32)   # elsewhere sigma is 0 by the construction of the bits
        self._master = torch.cat([sg[:, None], co], dim=1).contiguous()

    def _state(self):
        from . import _lib
        return _lib.KnerfBakedTrain(self.field._c, C.c_void_p(self._slot_of.data_ptr()), C.c_void_p(self._grad.data_ptr()), self.n_slots)

    def _apply_launch(self):
        from .runtime import _ptr
        return "knerf_baked_train_apply", (_ptr(self._point_of), _ptr(self._trainable))

    def _tv_launch(self):
        from .runtime import _ptr
        return "knerf_baked_train_tv", (_ptr(self._point_of), _ptr(self._master)), self.n_slots

    # ---- views for tests and tools
    def gradients(self):
        """(g_sigma [Rx,Ry,Rz], g_coef [Rx,Ry,Rz,K,3]): dense fp32 copies of the accumulated gradient, zero outside the slots"""
        import torch
        res, K = self.field.resolution, n_coefficients(self.field.sh_degree)
        P = int(np.prod(res))
        gs = torch.zeros((P,), device=self.field.device, dtype=torch.float32)
        gc = torch.zeros((P, 3 * K), device=self.field.device, dtype=torch.float32)
        gs[self._index] = self._grad[:, 0]
        gc[self._index] = self._grad[:, 1:]
        return gs.reshape(res), gc.reshape(res + (K, 3))

    @property
    def slot_mask(self):
        """bool [Rx,Ry,Rz] on the device: the lattice points that have a slot"""
        return (self._slot_of >= 0).reshape(self.field.resolution)

    @property
    def sigma_trainable(self):
        """bool [Rx,Ry,Rz] on the device: the lattice points whose sigma the optimiser may change"""
        import torch
        out = torch.zeros((self._slot_of.numel(),), device=self.field.device, dtype=torch.bool)
        out[self._index] = self._trainable.bool()
        return out.reshape(self.field.resolution)

    def finish(self, sigma_threshold=None):
        """An ordinary BakedField from the live one: every sigma <= sigma_threshold (default: the field's own) stored as 0 and the
        occupancy bits rebuilt from sigma (a subset of the support, so skipping stays exact).  The optimiser stays usable."""
        import torch
        from .runtime import occupancy_words_from_grid
        f = self.field
        thr = f.sigma_threshold if sigma_threshold is None else check_threshold(sigma_threshold)
        sigma = f.sigma
        sigma = torch.where(sigma > thr, sigma, torch.zeros_like(sigma)).contiguous()
        records = f._records.clone()
        records[:, :4] = sigma.reshape(-1, 1).view(torch.uint8)
        words = occupancy_words_from_grid(sigma, 0.0, 0, what="BakedFieldOptimizer.finish")
        return BakedField(records, words, f.resolution, f.bounds, f.sh_degree, thr)


@takes_depth_loss
def brick_optimizer(field, learning_rate_sigma, learning_rate_sh, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dilation=0, step=None,
                    white_background=False, termination=0.0, lanes_per_ray=0, loss=None, regularizers=None, background=None,
                    opacity_loss=0.0, target_background=None, background_seed=0):
    """A BrickFieldOptimizer (baked_bricks_train.py) over a COPY of a BrickBakedField's bricks: BakedField.optimizer for a field
    stored as sparse bricks, with the same arguments and meaning, optimised as it is (no table of the dense lattice's size is formed;
    finish() gives a BrickBakedField).  There is no total-variation regulariser here: tv_sigma, tv_sh and tv_epsilon belong to the
    dense optimiser and, on bricks, to baked_bricks_grow.grid_trainer, beside resample_bricks and fit_coarse_to_fine_bricks.
    loss, regularizers: the objective, as BakedField.optimizer takes it (knerf_baked_bricks_train_rays_ext); background, opacity_loss,
    target_background, background_seed: the rgba keywords, as there (knerf_baked_bricks_train_rays_rgba); depth_loss: the weight of the
    depth term, as there (knerf_baked_bricks_train_rays_depth)."""
    from .baked_bricks_train import BrickFieldOptimizer
    from .baked_quant import QuantizedBrickField
    if isinstance(field, QuantizedBrickField):
        raise ValueError("a brick optimiser is built on a BrickBakedField, got a QuantizedBrickField: dequantize() gives one")
    return BrickFieldOptimizer(field, learning_rate_sigma=learning_rate_sigma, learning_rate_sh=learning_rate_sh, beta_1=beta_1,
                               beta_2=beta_2, epsilon=epsilon, dilation=dilation, step=step, white_background=white_background,
                               termination=termination, lanes_per_ray=lanes_per_ray, loss=loss, regularizers=regularizers,
                               background=background, opacity_loss=opacity_loss, target_background=target_background,
                               background_seed=background_seed)


def __getattr__(name):
    """the brick optimiser's names live in baked_bricks_train.py (which imports this module) and are reachable from here as well"""
    if name in ("BrickFieldOptimizer", "BRICK_TRAIN_VARIANTS"):
        from . import baked_bricks_train
        return getattr(baked_bricks_train, name)
    if name in ("BrickGridTrainer", "grid_trainer", "resample_bricks", "fit_coarse_to_fine_bricks"):
        from . import baked_bricks_grow       # (it imports this module as well)
        return getattr(baked_bricks_grow, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def check_stages(stages):
    """ValueError unless stages is a non-empty sequence of (resolution | None, steps) with steps a non-negative integer; returns
    them as a list of (resolution | None, int).  The resolutions themselves are checked by BakedField.resample."""
    try:
        out = [(r, s) for r, s in stages]
    except (TypeError, ValueError):
        raise ValueError(f"stages must be a sequence of (resolution | None, steps), got {stages!r}") from None
    if not out:
        raise ValueError("stages must name at least one stage")
    for r, s in out:
        if not is_number(s, integer=True) or int(s) < 0:
            raise ValueError(f"the steps of a stage must be a non-negative integer, got {s!r}")
    return [(r, int(s)) for r, s in out]


class StageBatches:
    """At most `steps` further batches of an iterator `it` over `batches`, for one stage's fit(): what itertools.islice gives, with the
    source's last_depth (RayBatchDataset.set_depth) still readable after each batch is drawn"""

    def __init__(self, batches, it, steps):
        self._batches, self._it, self._steps = batches, it, int(steps)

    @property
    def last_depth(self):
        return getattr(self._batches, "last_depth", None)

    def __iter__(self):
        import itertools
        return itertools.islice(self._it, self._steps)


def fit_coarse_to_fine(field, batches, near, far, stages, **optimizer_kwargs):
    """Coarse-to-fine optimisation of a baked field: for every stage (resolution | None, steps) in turn the field is resampled onto
    `resolution` (BakedField.resample; None keeps the lattice), an optimiser is built on it (field.optimizer(**optimizer_kwargs):
    learning rates, dilation, march, total-variation and objective (loss=, regularizers=) keywords), fit for `steps` batches and finished (finish()).  `batches` is
    consumed continuously: a stage goes on where the one before stopped, and no batch is dropped in between.  Its last_depth, where it
    has one (RayBatchDataset.set_depth), reaches every step: with depth_loss= among the keywords the stages are depth-supervised.

    Adam's moments are NOT carried across stages.  A resample changes the lattice, the support and with them the set of slots, so
    every stage gets a new slot set and a fresh optimiser whose moments start at zero and whose bias correction starts at t = 1.

    Returns (the finished field of the last stage, history): history["loss"] (and "tv_sigma", "tv_sh" when a weight is > 0, and the four
    lists of objective_terms() under an objective that is not the plain one) run over all stages, history["stages"] holds one {"resolution", "steps", "n_slots"} per stage (steps: those actually run)."""
    todo = check_stages(stages)
    it = iter(batches)
    history = {"loss": [], "stages": []}
    for resolution, steps in todo:
        if resolution is not None:
            field = field.resample(resolution)
        opt = field.optimizer(**optimizer_kwargs)
        hist = opt.fit(StageBatches(batches, it, steps), near, far)
        for key, values in hist.items():
            history.setdefault(key, []).extend(values)
        history["stages"].append({"resolution": tuple(field.resolution), "steps": len(hist["loss"]), "n_slots": opt.n_slots})
        field = opt.finish()
    return field, history
