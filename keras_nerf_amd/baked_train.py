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

from .baked import BakedField, _check, _ray_args, _stream, _unpack_words, check_render_args, check_threshold, n_coefficients


def check_optimizer_args(learning_rate_sigma, learning_rate_sh, beta_1, beta_2, epsilon, dilation):
    """ValueError unless both learning rates and epsilon are finite and > 0, both betas lie in [0, 1) and dilation is an integer 0..8
    (what knerf_occupancy_from_grid takes); returns them as (float, float, float, float, float, int)"""
    def number(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(float(v)):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        return float(v)
    lrs, lrc = number("learning_rate_sigma", learning_rate_sigma), number("learning_rate_sh", learning_rate_sh)
    b1, b2, eps = number("beta_1", beta_1), number("beta_2", beta_2), number("epsilon", epsilon)
    if not (lrs > 0.0 and lrc > 0.0):
        raise ValueError(f"learning rates must be > 0, got {learning_rate_sigma!r} and {learning_rate_sh!r}")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"beta_1 and beta_2 must lie in [0, 1), got {beta_1!r} and {beta_2!r}")
    if not np.float32(eps) > 0.0:
        raise ValueError(f"epsilon must be > 0 (as a float32), got {epsilon!r}")
    if isinstance(dilation, bool) or not isinstance(dilation, (int, np.integer)) or not 0 <= int(dilation) <= 8:
        raise ValueError(f"dilation must be an integer 0..8, got {dilation!r}")
    return lrs, lrc, b1, b2, eps, int(dilation)


def check_tv_args(tv_sigma, tv_sh, tv_epsilon):
    """ValueError unless both total-variation weights are finite and >= 0 and tv_epsilon is finite and > 0 (as a float32); returns
    them as floats"""
    out = []
    for name, v in (("tv_sigma", tv_sigma), ("tv_sh", tv_sh), ("tv_epsilon", tv_epsilon)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(np.float32(v)):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        out.append(float(v))
    if out[0] < 0.0 or out[1] < 0.0:
        raise ValueError(f"tv_sigma and tv_sh must be >= 0, got {tv_sigma!r} and {tv_sh!r}")
    if not np.float32(out[2]) > 0.0:
        raise ValueError(f"tv_epsilon must be > 0 (as a float32), got {tv_epsilon!r}")
    return tuple(out)


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


def objective_value(obj, terms, norm):
    """(loss, {name: mean}) from the per-ray terms [n, 4] of an extended launch, float64 device scalars: the terms are summed in float64
    on the device; photometric and mse are means over rays and channels, distortion and opacity_entropy over rays (N = norm); loss =
    photometric + distortion weight x mean D + opacity_entropy weight x mean H, the function whose gradient the launch added."""
    import torch
    total = terms.to(torch.float64).sum(dim=0)
    n = float(max(norm, 1))
    means = {"photometric": total[0] / (3.0 * n), "mse": total[1] / (3.0 * n), "distortion": total[2] / n,
             "opacity_entropy": total[3] / n}
    loss = means["photometric"] + float(obj.distortion) * means["distortion"] + float(obj.opacity_entropy) * means["opacity_entropy"]
    return loss, means


def fit_terms(out, rows):
    """adds the four lists of TERM_NAMES (with "opacity" behind them where the steps were rgba launches) to a fit() dict from the
    per-step objective_terms() (one device read)"""
    import torch
    names = TERM_NAMES + (("opacity",) if rows and all("opacity" in r for r in rows) else ())
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
        if isinstance(opacity_loss, bool) or not isinstance(opacity_loss, (int, float, np.floating, np.integer)) or \
                not np.isfinite(np.float32(opacity_loss)) or float(opacity_loss) < 0.0:
            raise ValueError(f"opacity_loss must be a finite number >= 0, got {opacity_loss!r}")
        self.opacity = float(opacity_loss)
        if target_background not in (None, "black", "white"):
            raise ValueError(f'target_background must be None, "black" or "white", got {target_background!r}')
        self.stored = float(white) if target_background is None else float(target_background == "white")
        if isinstance(background_seed, bool) or not isinstance(background_seed, (int, np.integer)):
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
    total = terms.to(torch.float64).sum(dim=0)
    n = float(max(norm, 1))
    means = {"photometric": total[0] / (3.0 * n), "mse": total[1] / (3.0 * n), "distortion": total[2] / n,
             "opacity_entropy": total[3] / n, "opacity": total[4] / n}
    loss = means["photometric"] + float(rec.opacity) * means["opacity"]
    if obj is not None:
        loss = loss + float(obj.distortion) * means["distortion"] + float(obj.opacity_entropy) * means["opacity_entropy"]
    return loss, means


def bias_corrected_rate(learning_rate: float, beta_1: float, beta_2: float, t: int) -> float:
    """Keras-form Adam: learning_rate sqrt(1 - beta_2^t) / (1 - beta_1^t) in double, t the step being applied (from 1)"""
    return float(learning_rate) * float(np.sqrt(1.0 - float(beta_2) ** t)) / (1.0 - float(beta_1) ** t)


class BakedFieldOptimizer:
    """Adam on the records of a baked field (BakedField.optimizer builds one).  `field` is the live field: it owns the records the
    optimiser rewrites, its bits are the support, and it can be rendered at any time."""

    _rgba = RgbaTargets()               # the rgba keywords at their defaults: every launch is what it was without them

    def __init__(self, source, learning_rate_sigma, learning_rate_sh, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dilation=0, step=None,
                 white_background=False, termination=0.0, lanes_per_ray=0, tv_sigma=0.0, tv_sh=0.0, tv_epsilon=1e-6, loss=None,
                 regularizers=None, background=None, opacity_loss=0.0, target_background=None, background_seed=0):
        import torch
        from . import _lib
        from .runtime import occupancy_words_from_grid
        self._rgba = RgbaTargets(white_background, background, opacity_loss, target_background, background_seed)
        self.learning_rate_sigma, self.learning_rate_sh, self.beta_1, self.beta_2, self.epsilon, self.dilation = \
            check_optimizer_args(learning_rate_sigma, learning_rate_sh, beta_1, beta_2, epsilon, dilation)
        self.tv_sigma, self.tv_sh, self.tv_epsilon = check_tv_args(tv_sigma, tv_sh, tv_epsilon)
        self.objective = check_objective(loss, regularizers)               # None: the plain objective, the plain entry point
        self._terms = None                                                  # the last accumulate's means (objective_terms)
        self.last_regularizer = None                                        # what the latest train_step's regularize() returned
        check_render_args(step, termination, ("image",), source.sh_degree, lanes_per_ray)
        self.step, self.white_background, self.termination, self.lanes_per_ray = step, self._rgba.white, float(termination), \
            int(lanes_per_ray)
        dev, res, deg = source.device, source.resolution, source.sh_degree
        K = n_coefficients(deg)
        self._width = 1 + 3 * K
        sigma = source.sigma
        support = occupancy_words_from_grid(sigma, 0.0, self.dilation, what="BakedField.optimizer")
        self.field = BakedField(source._records.clone(), support, res, source.bounds, deg, source.sigma_threshold)
        cells = tuple(r - 1 for r in res)
        occ = _unpack_words(support, cells)
        cx, cy, cz = cells
        touched = torch.zeros(res, device=dev, dtype=torch.bool)
        # a point's sigma is trainable when none of its 8 adjacent cells is a lattice cell outside the support
        free = torch.ones(res, device=dev, dtype=torch.bool)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    touched[a:a + cx, b:b + cy, c:c + cz] |= occ
                    free[a:a + cx, b:b + cy, c:c + cz] &= occ
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
        self._grad = torch.zeros_like(self._master)
        self._m, self._v = torch.zeros_like(self._master), torch.zeros_like(self._master)
        self.iterations = 0                                                 # steps applied; the host's count, no device read
        self._c = _lib.KnerfBakedTrain(self.field._c, C.c_void_p(self._slot_of.data_ptr()), C.c_void_p(self._grad.data_ptr()),
                                       self.n_slots)

    # ---- the two launches
    def accumulate(self, origins, directions, near, far, target, n_total=None, background=None):
        """knerf_baked_train_rays: adds the gradient of the batch's mean squared error to the gradient rows and returns the loss, a
        float64 device scalar (the per-ray errors are summed in float64 on the device; nothing waits).  n_total: the N of the loss
        1 / (3 N) sum (out - target)^2 when the batch is one part of several accumulated before apply() (default: this batch's rays).
        With a loss= / regularizers= objective that is not the plain one: knerf_baked_train_rays_ext, and the value returned is that
        of the function whose gradient was added, the mean of rho plus distortion x mean D plus opacity_entropy x mean H (the per-ray
        terms summed in float64 on the device); objective_terms() then gives the four means.
        With the rgba keywords (background=, opacity_loss=), an [n,4] target (the fourth column is the photograph's alpha) or a
        per-call `background` ([n,3], values in [0,1], overrides the keyword): knerf_baked_train_rays_rgba, the prediction and the
        photograph composited over the ray's own background and opacity_loss x mean (O - alpha)^2 added; objective_terms() then has
        a fifth mean, "opacity", and last_background is the background tensor of the launch."""
        import torch
        from . import _lib
        from .runtime import _f32, _ptr
        f = self.field
        o, d, n, h, (near_t, near0), (far_t, far0) = _ray_args(f, origins, directions, near, far, self.step)
        tg, alpha = self._rgba.split_target(_f32(target, f.device), n)
        rgba = self._rgba.record(alpha, n, f.device, background)
        norm = n if n_total is None else int(n_total)
        if norm < 1 and n:
            raise ValueError(f"n_total must be a positive ray count, got {n_total!r}")
        sq = torch.empty((n,), device=f.device, dtype=torch.float32)
        flags = (_lib.BAKED_WHITE_BACKGROUND if self.white_background else 0) | _lib.BAKED_SKIP_EMPTY | \
            (self.lanes_per_ray << _lib.BAKED_LANES_SHIFT)
        if rgba is not None:
            terms = torch.zeros((n, 5), device=f.device, dtype=torch.float32)
            if n:
                _check(_lib.load().knerf_baked_train_rays_rgba(_stream(f.device), C.byref(self._c), _ptr(o), _ptr(d), _ptr(near_t),
                                                               _ptr(far_t), near0, far0, _ptr(tg), n, norm, h, self.termination, flags,
                                                               _ptr(sq), C.byref(self.objective) if self.objective is not None else None,
                                                               _ptr(terms), C.byref(rgba)), "knerf_baked_train_rays_rgba")
            loss, self._terms = rgba_value(self.objective, rgba, terms, norm)
            return loss
        if self.objective is not None:
            terms = torch.zeros((n, 4), device=f.device, dtype=torch.float32)
            if n:
                _check(_lib.load().knerf_baked_train_rays_ext(_stream(f.device), C.byref(self._c), _ptr(o), _ptr(d), _ptr(near_t),
                                                              _ptr(far_t), near0, far0, _ptr(tg), n, norm, h, self.termination, flags,
                                                              _ptr(sq), C.byref(self.objective), _ptr(terms)),
                       "knerf_baked_train_rays_ext")
            loss, self._terms = objective_value(self.objective, terms, norm)
            return loss
        if n:
            _check(_lib.load().knerf_baked_train_rays(_stream(f.device), C.byref(self._c), _ptr(o), _ptr(d), _ptr(near_t), _ptr(far_t),
                                                      near0, far0, _ptr(tg), n, norm, h, self.termination, flags, _ptr(sq)),
                   "knerf_baked_train_rays")
        return sq.to(torch.float64).sum() / (3.0 * max(norm, 1))

    def objective_terms(self):
        """{"photometric", "mse", "distortion", "opacity_entropy"}: the four means of the last accumulate() as float64 device scalars
        (photometric: the mean of rho over rays and channels; mse: of the squared difference; the other two: mean D and mean H over
        the rays, unweighted); after an rgba launch also "opacity", the mean of (O - alpha)^2 over the rays, unweighted.  None before
        any accumulate(), and always under the plain objective without the rgba keywords."""
        return None if self._terms is None else dict(self._terms)

    @property
    def last_background(self):
        """the background tensor [n,3] of the last accumulate() (None: the launch used the flag's colour)"""
        return self._rgba.last_background

    def apply(self):
        """knerf_baked_train_apply: one Adam step from the accumulated gradient, the records rewritten, the gradient zeroed"""
        from . import _lib
        from .runtime import _ptr
        t = self.iterations + 1
        _check(_lib.load().knerf_baked_train_apply(
            _stream(self.field.device), C.byref(self._c), _ptr(self._point_of), _ptr(self._trainable), _ptr(self._master), _ptr(self._m),
            _ptr(self._v), bias_corrected_rate(self.learning_rate_sigma, self.beta_1, self.beta_2, t),
            bias_corrected_rate(self.learning_rate_sh, self.beta_1, self.beta_2, t), self.beta_1, self.beta_2, self.epsilon),
            "knerf_baked_train_apply")
        self.iterations = t

    @property
    def regularized(self) -> bool:
        """whether a total-variation weight is > 0: train_step then runs regularize() between accumulate() and apply()"""
        return self.tv_sigma > 0.0 or self.tv_sh > 0.0

    def tv_weights(self):
        """the weights per term knerf_baked_train_tv takes, formed in double: tv_sigma / n_slots and tv_sh / (3 K n_slots)"""
        return self.tv_sigma / float(self.n_slots), self.tv_sh / (float(self._width - 1) * float(self.n_slots))

    def regularize(self):
        """knerf_baked_train_tv, one launch: adds the gradient of R = tv_sigma mean_p tv_sigma(p) + tv_sh mean_{p,q} tv_q(p) (the total
        variation of the master values over the slots, include/knerf.h) to the gradient rows and returns the two means, unweighted,
        as float64 device scalars (the per-slot terms are summed in float64 on the device; nothing waits)."""
        import torch
        from . import _lib
        from .runtime import _ptr
        dev = self.field.device
        tv = torch.empty((self.n_slots, 2), device=dev, dtype=torch.float32)
        ws, wc = self.tv_weights()
        _check(_lib.load().knerf_baked_train_tv(_stream(dev), C.byref(self._c), _ptr(self._point_of), _ptr(self._master), ws, wc,
                                                self.tv_epsilon, _ptr(tv)), "knerf_baked_train_tv")
        total = tv.to(torch.float64).sum(dim=0)
        return total[0] / float(self.n_slots), total[1] / (float(self._width - 1) * float(self.n_slots))

    def train_step(self, origins, directions, near, far, target):
        """accumulate, regularize (only when a total-variation weight is > 0; its return value is kept in last_regularizer), apply;
        returns the batch's loss before the step (float64 device scalar, the data term alone)"""
        loss = self.accumulate(origins, directions, near, far, target)
        if self.regularized:
            self.last_regularizer = self.regularize()
        self.apply()
        return loss

    def fit(self, batches, near, far, steps=None):
        """train_step on every batch of `batches` (each (target [n,3], (origins, directions, t)) as RayBatchDataset yields them; t is
        not used: the baked march places its own samples), at most `steps` of them.  {"loss": [...]}: read from the device once, after
        the last step.  With a total-variation weight > 0 the dict also holds "tv_sigma" and "tv_sh": regularize()'s two means per
        step; with an objective that is not the plain one also "photometric", "mse", "distortion" and "opacity_entropy":
        objective_terms() per step, and "opacity" behind them where the steps were rgba launches."""
        import torch
        if steps is not None and (isinstance(steps, bool) or int(steps) != steps or int(steps) < 0):
            raise ValueError(f"steps must be a non-negative integer or None, got {steps!r}")
        losses, tvs, terms = [], [], []
        for k, (target, (o, d, _t)) in enumerate(batches):
            if steps is not None and k >= int(steps):
                break
            losses.append(self.train_step(o, d, near, far, target))
            if self.regularized:
                tvs.append(torch.stack(self.last_regularizer))
            if self._terms is not None:
                terms.append(self.objective_terms())
        out = {"loss": torch.stack(losses).cpu().tolist() if losses else []}
        if self.regularized:
            both = torch.stack(tvs).cpu() if tvs else torch.zeros((0, 2))
            out["tv_sigma"], out["tv_sh"] = both[:, 0].tolist(), both[:, 1].tolist()
        if self.objective is not None or terms:
            fit_terms(out, terms)
        return out

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


def brick_optimizer(field, learning_rate_sigma, learning_rate_sh, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dilation=0, step=None,
                    white_background=False, termination=0.0, lanes_per_ray=0, loss=None, regularizers=None, background=None,
                    opacity_loss=0.0, target_background=None, background_seed=0):
    """A BrickFieldOptimizer (baked_bricks_train.py) over a COPY of a BrickBakedField's bricks: BakedField.optimizer for a field
    stored as sparse bricks, with the same arguments and meaning, optimised as it is (no table of the dense lattice's size is formed;
    finish() gives a BrickBakedField).  There is no total-variation regulariser here: tv_sigma, tv_sh and tv_epsilon belong to the
    dense optimiser and, on bricks, to baked_bricks_grow.grid_trainer, beside resample_bricks and fit_coarse_to_fine_bricks.
    loss, regularizers: the objective, as BakedField.optimizer takes it (knerf_baked_bricks_train_rays_ext); background, opacity_loss,
    target_background, background_seed: the rgba keywords, as there (knerf_baked_bricks_train_rays_rgba)."""
    from .baked_bricks_train import BrickFieldOptimizer
    from .baked_quant import QuantizedBrickField
    if isinstance(field, QuantizedBrickField):
        raise ValueError("a brick optimiser is built on a BrickBakedField, got a QuantizedBrickField: dequantize() gives one")
    return BrickFieldOptimizer(field, learning_rate_sigma, learning_rate_sh, beta_1, beta_2, epsilon, dilation, step, white_background,
                               termination, lanes_per_ray, loss, regularizers, background, opacity_loss, target_background,
                               background_seed)


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
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or int(s) < 0:
            raise ValueError(f"the steps of a stage must be a non-negative integer, got {s!r}")
    return [(r, int(s)) for r, s in out]


def fit_coarse_to_fine(field, batches, near, far, stages, **optimizer_kwargs):
    """Coarse-to-fine optimisation of a baked field: for every stage (resolution | None, steps) in turn the field is resampled onto
    `resolution` (BakedField.resample; None keeps the lattice), an optimiser is built on it (field.optimizer(**optimizer_kwargs):
    learning rates, dilation, march, total-variation and objective (loss=, regularizers=) keywords), fit for `steps` batches and finished (finish()).  `batches` is
    consumed continuously: a stage goes on where the one before stopped, and no batch is dropped in between.

    Adam's moments are NOT carried across stages.  A resample changes the lattice, the support and with them the set of slots, so
    every stage gets a new slot set and a fresh optimiser whose moments start at zero and whose bias correction starts at t = 1.

    Returns (the finished field of the last stage, history): history["loss"] (and "tv_sigma", "tv_sh" when a weight is > 0, and the four
    lists of objective_terms() under an objective that is not the plain one) run over all stages, history["stages"] holds one {"resolution", "steps", "n_slots"} per stage (steps: those actually run)."""
    import itertools
    todo = check_stages(stages)
    it = iter(batches)
    history = {"loss": [], "stages": []}
    for resolution, steps in todo:
        if resolution is not None:
            field = field.resample(resolution)
        opt = field.optimizer(**optimizer_kwargs)
        hist = opt.fit(itertools.islice(it, steps), near, far)
        for key, values in hist.items():
            history.setdefault(key, []).extend(values)
        history["stages"].append({"resolution": tuple(field.resolution), "steps": len(hist["loss"]), "n_slots": opt.n_slots})
        field = opt.finish()
    return field, history
