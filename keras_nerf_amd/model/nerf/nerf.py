"""NeRF -- counterpart of reference keras_nerf/model/nerf/nerf.py:10-508 on the MI355X hot path.

Same constructor / compile / fit / train_step / test_step / predict_and_render_* / save_model / load_model surface and
the same chunk semantics (equal ray chunks, mean of chunk losses, one optimizer step per batch, divisibility assert);
the per-chunk body runs in hand-written HIP behind the C ABI (include/knerf.h).  Data parallelism is one process per GPU:
when torch.distributed is initialised, the accumulated gradients of both MLPs are all-reduced (SUM, as Keras optimizers
aggregate under MirroredStrategy -- reference train.py:75, nerf.py:455-458) over RCCL before the two Adam updates.
"""
from __future__ import annotations

import json
import logging
import os
from typing import Dict, Optional

import numpy as np
import torch

from ... import losses as _losses
from ... import optimizers, parallel
from ...runtime import COARSE, FINE, OCCUPANCY_OUTSIDE, KnerfContext, NonFiniteGradientError, marching_cubes, occupancy_from_grid, occupancy_spec  # noqa: F401
from .metrics import RAY_NAMES, Mean, MetricLogs, MetricState
from .mlp import NeRFMLP
from .utils import NeRFUtils


def _is_mse(loss) -> bool:
    """The fused kernels implement the reference's loss, mean squared error over [R,3] (train_single.py:127,
    train.py:130-136).  Strings / None are accepted by name; a callable is probed numerically."""
    if loss is None or (isinstance(loss, str) and loss.lower() in ("mse", "mean_squared_error", "meansquarederror")):
        return True
    if callable(loss):
        a = torch.linspace(0, 1, 24).reshape(8, 3); b = torch.flip(a, [0]) * 0.5
        try:
            v = float(torch.as_tensor(loss(a, b)))
        except Exception:
            return False
        return abs(v - float(torch.mean((a - b) ** 2))) < 1e-6
    return False


def _adam_hyper(optimizer) -> Dict[str, float]:
    """tf.keras.optimizers.get('adam') defaults (nerf.py:163-165); a dict or an object with the Keras attribute names
    overrides them.  Only PLAIN Adam with a constant learning rate is implemented (what the reference trains with): any
    other optimizer, amsgrad, weight decay, gradient clipping, EMA or a learning-rate schedule is refused, not ignored."""
    h = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7)
    if optimizer is None or (isinstance(optimizer, str) and optimizer.lower() == "adam"):
        return h
    if isinstance(optimizer, str):
        raise ValueError(f"optimizer '{optimizer}': only Adam is implemented (the reference trains with 'adam')")
    cfg = {}
    if isinstance(optimizer, dict):
        cfg = dict(optimizer.get("config", optimizer))          # Keras serialised form {"class_name", "config"} or a flat dict
        name = str(optimizer.get("class_name", cfg.get("name", "adam")))
    else:
        name = type(optimizer).__name__
        if callable(getattr(optimizer, "get_config", None)):
            try:
                cfg = dict(optimizer.get_config())
            except Exception:
                cfg = {}
        for k in ("learning_rate", "lr", "beta_1", "beta_2", "epsilon", "amsgrad", "weight_decay", "clipnorm", "clipvalue",
                  "global_clipnorm", "use_ema"):
            if k not in cfg and getattr(optimizer, k, None) is not None:
                cfg[k] = getattr(optimizer, k)
        name = str(cfg.get("name", name))
    if name.lower() not in ("adam", "dict", "simplenamespace", "namespace"):
        raise ValueError(f"optimizer {name}: only plain Adam is implemented (the reference trains with 'adam')")
    for k in ("amsgrad", "weight_decay", "clipnorm", "clipvalue", "global_clipnorm", "use_ema"):
        if cfg.get(k) not in (None, False, 0, 0.0):
            raise ValueError(f"Adam option {k}={cfg[k]!r} is not implemented by the fused optimizer kernel")
    for src, dst in (("learning_rate", "lr"), ("lr", "lr"), ("beta_1", "beta1"), ("beta_2", "beta2"), ("epsilon", "epsilon")):
        v = cfg.get(src)
        if v is None:
            continue
        if isinstance(v, dict) or callable(v) or (hasattr(v, "get_config") and not hasattr(v, "__float__")):
            raise ValueError(f"Adam {src}: learning-rate schedules are not implemented (constant learning rate only)")
        try:
            h[dst] = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"Adam {src}={v!r} is not a number (learning-rate schedules are not implemented)") from None
    return h


_CLIP_OPTIONS = ("clipnorm", "clipvalue", "global_clipnorm")


def _optimizer_spec(optimizer) -> optimizers.OptimizerSpec:
    """What `compile(optimizer=...)` accepts: 'adam' / None, keras_nerf_amd.optimizers.Adam, any object with the Keras attribute names or
    a `get_config()` (a real tf.keras Adam), and the serialised form {"class_name", "config"} (schedules nested the same way).  Beyond
    plain Adam (`_adam_hyper`, which still supplies the four numbers): a learning rate that is an ExponentialDecay, CosineDecay or
    PiecewiseConstantDecay, ONE of clipnorm / clipvalue / global_clipnorm, and weight_decay (decoupled, the AdamW form of Keras' Adam).
    amsgrad, use_ema, gradient accumulation, other schedules, plain callables and other optimizers raise ValueError naming the option."""
    if optimizer is None or isinstance(optimizer, str):
        return optimizers.OptimizerSpec(**_adam_hyper(optimizer))
    if isinstance(optimizer, optimizers.OptimizerSpec):
        return optimizer
    cfg = {}
    if isinstance(optimizer, dict):
        cfg = dict(optimizer.get("config", optimizer))
        name = str(optimizer.get("class_name", cfg.get("name", "adam")))
    else:
        name = type(optimizer).__name__
        if callable(getattr(optimizer, "get_config", None)):
            try:
                cfg = dict(optimizer.get_config())
            except Exception:
                cfg = {}
        for k in ("learning_rate", "lr", "beta_1", "beta_2", "epsilon", "amsgrad", "weight_decay", "use_ema", "gradient_accumulation_steps") + _CLIP_OPTIONS:
            if k not in cfg and getattr(optimizer, k, None) is not None:
                cfg[k] = getattr(optimizer, k)
        name = str(cfg.get("name", name))
    for k in ("amsgrad", "use_ema"):
        if cfg.get(k) not in (None, False, 0, 0.0):
            raise ValueError(f"Adam option {k}={cfg[k]!r} is not implemented by the optimizer kernels")
    if cfg.get("gradient_accumulation_steps") not in (None, 0, 1):
        raise ValueError(f"Adam option gradient_accumulation_steps={cfg['gradient_accumulation_steps']!r} is not implemented")
    clips = [(k, cfg[k]) for k in _CLIP_OPTIONS if cfg.get(k) is not None]
    if len(clips) > 1:
        raise ValueError(f"Adam: only one of clipnorm, clipvalue and global_clipnorm may be set, got {' and '.join(k for k, _ in clips)}")
    lr_key = "learning_rate" if cfg.get("learning_rate") is not None else "lr"
    lr = cfg.get(lr_key)
    schedule = None
    if lr is not None and not hasattr(lr, "__float__") and not isinstance(lr, (int, float, np.integer, np.floating)):
        schedule = optimizers.schedule_from(lr, lr_key)                  # ValueError for unknown classes and plain callables
    # the plain part through _adam_hyper: its name check, its number parsing, its defaults
    plain = {k: cfg[k] for k in ("beta_1", "beta_2", "epsilon") if cfg.get(k) is not None}
    if schedule is None and lr is not None:
        plain["learning_rate"] = lr
    h = _adam_hyper({"class_name": name, "config": plain})
    wd = cfg.get("weight_decay")
    return optimizers.OptimizerSpec(lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"], epsilon=h["epsilon"], schedule=schedule,
                                    clip=clips[0][0] if clips else None, clip_arg=clips[0][1] if clips else 0.0,
                                    weight_decay=0.0 if wd in (None, False) else wd)


class History(dict):
    """what tf.keras.Model.fit returns: `.history` = {log key: [one value per epoch]}, `.epoch` = the epochs run, `.params`.  Also a
    dict itself (rounds 1-4 returned the plain dictionary), so both `h["fine_loss"]` and `h.history["fine_loss"]` read the curves."""

    def __init__(self, history, epoch, params):
        super().__init__(history)
        self.history, self.epoch, self.params = self, list(epoch), dict(params)


class NeRF:
    def __init__(self, n_coarse: int = 64, n_fine: int = 128, pos_emb_xyz: int = 10, pos_emb_dir: int = 4, n_layers: int = 8,
                 dense_units: int = 256, skip_layer=4, model_path: str = None, oob: str = "zero", seed: int = 42, **kwargs):
        logging.info("Initializing NeRF model")
        self.model_path = model_path
        if self.model_path is None:
            self.n_coarse, self.n_fine = n_coarse, n_fine
            self.pos_emb_xyz, self.pos_emb_dir = pos_emb_xyz, pos_emb_dir
            self.n_layers, self.dense_units, self.skip_layer = n_layers, dense_units, skip_layer
        else:
            self.load_model(model_path)                       # nerf.py:33-35: config comes from model_config.json
        # NB the reference builds the MLPs from the constructor arguments even when a model_path is given (nerf.py:37-40);
        # here the loaded config wins, which is what the saved weights need.
        xyz_dim, dir_dim = 3 + 6 * self.pos_emb_xyz, 3 + 6 * self.pos_emb_dir
        self.coarse = NeRFMLP(self.n_layers, self.dense_units, self.skip_layer, name="coarse_nerf", xyz_dim=xyz_dim,
                              dir_dim=dir_dim, seed=seed)
        self.fine = NeRFMLP(self.n_layers, self.dense_units, self.skip_layer, name="fine_nerf", xyz_dim=xyz_dim,
                            dir_dim=dir_dim, seed=seed + 1)
        self.oob = oob
        self.epsilon = 1e-10
        self.seed = seed
        self._ctx: Optional[KnerfContext] = None
        self._compiled = False
        self._global_step = 0
        self.stop_training = False

    # ------------------------------------------------------------------ save / load (nerf.py:45-76)
    def save_model(self, path, weights_only=False, optimizer_state=False):
        """nerf.py:45-64.  optimizer_state=True (extension; needs a compiled model) additionally writes optimizer_state.npz: the count
        of applied steps, Adam's m and v of both nets at their real widths and the optimizer configuration -- with the two weight files
        the whole state of a run (load_optimizer_state).  The default writes exactly the reference's files."""
        logging.info("Saving NeRF model")
        if optimizer_state and self._ctx is None:
            raise RuntimeError("save_model(optimizer_state=True): the model is not compiled, there is no optimizer state")
        if self._ctx is not None:
            self._ctx.poll_nonfinite(wait=True)      # never checkpoint past an unreported skipped step
        os.makedirs(path, exist_ok=True)
        if not weights_only:
            cfg = dict(n_coarse=self.n_coarse, n_fine=self.n_fine, pos_emb_xyz=self.pos_emb_xyz, pos_emb_dir=self.pos_emb_dir,
                       n_layers=self.n_layers, dense_units=self.dense_units, skip_layer=self.skip_layer)
            with open(os.path.join(path, "model_config.json"), "w") as f:
                json.dump(cfg, f)
        # same file names AND container as the reference: Keras-layout HDF5 (keras_nerf_amd/io/hdf5_min.py)
        self.coarse.save_weights(os.path.join(path, "coarse.h5"))
        self.fine.save_weights(os.path.join(path, "fine.h5"))
        if optimizer_state:
            (cm, cv), (fm, fv) = self._ctx.get_adam_state(COARSE), self._ctx.get_adam_state(FINE)
            optimizers.save_optimizer_state(path, self._ctx.step, dict(coarse_m=cm, coarse_v=cv, fine_m=fm, fine_v=fv),
                                            self._opt_spec.get_config())

    def load_optimizer_state(self, path):
        """After compile: Adam's slots and the step count from <path>/optimizer_state.npz (save_model(optimizer_state=True)), so that
        the next train_step continues the saved run bit for bit.  The optimizer itself is the one given to compile (the saved
        configuration is returned for the caller to compare); raises ValueError if the parameter counts differ."""
        if self._ctx is None:
            raise RuntimeError("load_optimizer_state: call compile(...) first")
        step, slots, config = optimizers.load_optimizer_state(path)
        n = self._ctx.param_count
        if slots["coarse_m"].size != n:
            raise ValueError(f"load_optimizer_state: the file holds {slots['coarse_m'].size} parameters per net, the model has {n}")
        self._ctx.poll_nonfinite(wait=True)
        self._ctx.set_adam_state(COARSE, slots["coarse_m"], slots["coarse_v"])
        self._ctx.set_adam_state(FINE, slots["fine_m"], slots["fine_v"])
        self._ctx.step = step
        return config

    @property
    def learning_rate(self) -> float:
        """the rate of the NEXT optimizer step: the schedule (in Python floats) at the host's count of applied steps"""
        if self._ctx is None:
            raise RuntimeError("the model is not compiled: call compile(...) first")
        return self._opt_spec.lr_at(self._ctx.step)

    def set_learning_rate(self, lr):
        """a new constant rate from the next step on (stream-ordered, nothing waits); constant schedules only"""
        if self._ctx is None:
            raise RuntimeError("the model is not compiled: call compile(...) first")
        sp = self._opt_spec
        if sp.schedule is not None:
            raise ValueError(f"set_learning_rate: the learning rate follows a {type(sp.schedule).__name__} schedule")
        new = optimizers.OptimizerSpec(lr=lr, beta1=sp.beta1, beta2=sp.beta2, epsilon=sp.epsilon, clip=sp.clip, clip_arg=sp.clip_arg,
                                       weight_decay=sp.weight_decay)
        self._ctx.set_optimizer(new)
        self._opt_spec = new

    def load_model(self, path):
        with open(os.path.join(path, "model_config.json"), "r") as f:
            c = json.load(f)
        self.n_coarse, self.n_fine = c["n_coarse"], c["n_fine"]
        self.pos_emb_xyz, self.pos_emb_dir = c["pos_emb_xyz"], c["pos_emb_dir"]
        self.n_layers, self.dense_units, self.skip_layer = c["n_layers"], c["dense_units"], c["skip_layer"]

    # ------------------------------------------------------------------ compile (nerf.py:78-173)
    def compile(self, optimizer="adam", loss="mse", batch_size=1, image_height=128, image_width=128, ray_chunks=2048,
                white_background=False, is_training=True, all_reduce="sum", deterministic=False, skip_dead_tiles=None,
                regularizers=None, **kwargs):
        """nerf.py:78-173.  Extensions (keyword-only in spirit; the reference's callers never pass them):
        all_reduce 'sum' | 'mean' (data parallel), deterministic (bit-reproducible gradient sums, slower),
        skip_dead_tiles (None = the library default, on, unless KNERF_SKIP_DEAD_TILES says otherwise: the backward skips 32-sample
        tiles whose dL/d(rgb, sigma) is exactly zero -- same gradients, less work once the scene has empty space).
        loss: besides mean squared error (by name, None, or a callable that computes it) what keras_nerf_amd.losses.loss_from takes --
        "mae", "huber", "log_cosh", the classes of that module, Keras loss objects of those classes and their serialised form; any
        other callable raises ValueError (it could not run inside the kernel).  regularizers: a losses.RayRegularizers (distortion and
        opacity-entropy terms of the rays' weights) or None."""
        logging.info("Compiling NeRF model")
        # validated before any context exists: a refused loss raises on a machine without a GPU too
        objective = _losses.objective_from(None if _is_mse(loss) else loss, regularizers)
        self.optimizer, self.loss = optimizer, loss
        self.batch_size, self.image_height, self.image_width = batch_size, image_height, image_width
        self.white_background = white_background
        self.run_eagerly = bool(kwargs.get("run_eagerly", False))
        self.ray_chunks = ray_chunks
        self.num_rays = batch_size * image_height * image_width
        if self.ray_chunks >= self.num_rays:                                      # nerf.py:95-98
            self.ray_chunks = self.num_rays
            logging.info(f"ray_chunks is greater than num_rays, setting ray_chunks to num_rays: {self.num_rays}")
        assert self.num_rays % self.ray_chunks == 0, \
            f"ray_chunks {self.ray_chunks} must be a divisor of the number of rays {self.num_rays}"   # nerf.py:100
        self.sequential_chunks = self.num_rays // self.ray_chunks
        if all_reduce not in ("sum", "mean"):
            raise ValueError("all_reduce must be 'sum' (Keras/MirroredStrategy semantics) or 'mean'")
        self.all_reduce = all_reduce
        spec = _optimizer_spec(optimizer)
        h = dict(lr=spec.lr, beta1=spec.beta1, beta2=spec.beta2, epsilon=spec.epsilon)
        if self._ctx is not None:
            self.coarse._host, self.fine._host = self.coarse.get_flat_weights(), self.fine.get_flat_weights()
            self.coarse._ctx = self.fine._ctx = None
            self._ctx.close()
        opts = {}
        if deterministic:
            opts["deterministic"] = 1
        if self.run_eagerly:                             # nerf.py:430-451: the zero-gradient check exists in eager mode only
            opts["grad_diagnostics"] = 1
        if skip_dead_tiles is not None:                  # only an explicit argument overrides KNERF_SKIP_DEAD_TILES (runtime.py)
            opts["skip_dead_tiles"] = int(bool(skip_dead_tiles))
        self._ctx = KnerfContext(self.n_coarse, self.n_fine, self.pos_emb_xyz, self.pos_emb_dir, self.n_layers, self.dense_units,
                                 self.skip_layer, white_background, self.oob, h["lr"], h["beta1"], h["beta2"], h["epsilon"],
                                 options=opts)
        self._opt_spec = spec
        if not spec.is_plain:                            # schedules, clipping, weight decay: csrc/optim_ext.hip (plain Adam never goes there)
            self._ctx.set_optimizer(spec)
        self._objective = objective
        self._loss_fn = _losses.loss_from(None if _is_mse(loss) else loss)
        self._objective_plain = _losses.is_plain(objective)
        if not self._objective_plain:                    # other losses, regularisers: csrc/composite_ext.hip (plain mse never goes there)
            self._ctx.set_objective(objective)
        self.device = self._ctx.device
        self.nerf_utils = NeRFUtils(batch_size, image_height, image_width, self.ray_chunks, self.pos_emb_xyz, self.pos_emb_dir,
                                    white_background, self.oob)
        self._build_model()
        self.is_training = is_training
        self._dist = parallel.is_distributed()
        if self._dist:                                   # mirrored variables start identical (train.py:110-148)
            parallel.broadcast_weights([self._ctx.weights_view(COARSE), self._ctx.weights_view(FINE)])
            self._ctx.refresh_weights()
        self._loss_acc = torch.zeros(2, device=self.device)
        self._initialize_metrics()
        self._diag_seen = 0
        self._compiled = True

    def _zero_gradient_diagnostics(self, wait: bool):
        """nerf.py:430-451 (eager mode only): the non-zero counts of the LAST chunk's coarse and fine gradients, counted on the
        device (knerf_grad_diagnostics), with the reference's three messages.  wait=False (the asynchronous `fit` path) reports the
        newest step that has completed, once.  One further message the reference cannot give: every 32-sample tile of a net's
        passes was exactly dead in the backward (knerf_tile_stats_net) -- the sigma == 0 collapse in which the ReLU on sigma is
        closed everywhere and no gradient can ever re-open it."""
        c, f, seq = self._ctx.grad_diagnostics(wait=wait)
        if seq == self._diag_seen:
            return None
        self._diag_seen = seq
        if c == 0 and f == 0:
            logging.error('Both Coarse and Fine Gradient are zero')
        elif c == 0:
            logging.warning('Coarse Gradient is zero')
        elif f == 0:
            logging.warning('Fine Gradient is zero')
        if wait and self._ctx.get_option("skip_dead_tiles_active"):
            # this step's share of the RUNNING totals: read without resetting them -- tile_stats() consumers (bench.py's dead_tile_frac,
            # fit's per-epoch report, tools/) accumulate across steps -- and difference against the previous read
            now = self._ctx.tile_stats_net(reset=False)
            prev = getattr(self, "_tile_stats_seen", ((0, 0), (0, 0)))
            self._tile_stats_seen = now
            for name, (l1, t1), (l0, t0) in zip(("coarse", "fine"), now, prev):
                if t1 < t0:                       # somebody reset the counters in between: the totals ARE the delta
                    l0 = t0 = 0
                live, total = l1 - l0, t1 - t0
                if total > 0 and live == 0:
                    logging.warning(f'Every sample tile of the {name} passes is dead (no sample passes a gradient): sigma has collapsed to zero '
                                    f'or the pixel error is exactly zero everywhere')
        return c, f

    def _build_model(self):                              # nerf.py:116-136
        self.coarse._bind(self._ctx, COARSE)
        self.fine._bind(self._ctx, FINE)
        if self.model_path is not None:
            logging.info("Loading NeRF model weights")
            self.coarse.load_weights(os.path.join(self.model_path, "coarse.h5"))
            self.fine.load_weights(os.path.join(self.model_path, "fine.h5"))

    def _initialize_metrics(self):                       # nerf.py:167-173
        # the six running means share one device-side state (metrics.py): a step enqueues its contribution, nothing is read back
        st = self._metric_state = MetricState(self.device)
        self.coarse_loss_tracker = Mean("coarse_loss", st, 0); self.coarse_psnr_metric = Mean("coarse_psnr", st, 1)
        self.corase_ssim_metric = Mean("coarse_ssim", st, 2)
        self.fine_loss_tracker = Mean("fine_loss", st, 3); self.fine_psnr_metric = Mean("fine_psnr", st, 4)
        self.fine_ssim_metric = Mean("fine_ssim", st, 5)

    @property
    def metrics(self):                                   # nerf.py:499-508
        return [self.coarse_loss_tracker, self.coarse_psnr_metric, self.corase_ssim_metric,
                self.fine_loss_tracker, self.fine_psnr_metric, self.fine_ssim_metric]

    @property
    def metrics_names(self):
        return [m.name for m in self.metrics]

    def reset_metrics(self):
        self._metric_state.state.zero_()

    # ------------------------------------------------------------------ forward
    def _flat_rays(self, rays):
        o, d, t = rays
        f = self._ctx.f32
        return f(o).reshape(self.num_rays, 3), f(d).reshape(self.num_rays, 3), f(t).reshape(self.num_rays, self.n_coarse)

    def _next_seed(self):
        self._global_step += 1
        rank = torch.distributed.get_rank() if getattr(self, "_dist", False) else 0
        return (self.seed << 20) ^ (rank << 40) ^ self._global_step        # replicas draw different u

    def _predict_and_render_chunk(self, ray_chunks, coarse_weights_chunk=None, u=None, seed=0):
        """nerf.py:175-216.  ray_chunks = (o [R,3], d [R,3], t_coarse [R,n_coarse])."""
        o, d, t = [self._ctx.f32(x) for x in ray_chunks]
        net = COARSE
        if coarse_weights_chunk is not None:
            t = self._ctx.sample_fine(t, coarse_weights_chunk, u, seed=seed)
            net = FINE
        image, depth, weights = self._ctx.forward_chunk(net, o, d, t)
        return {"image": image, "depth": depth, "weights": weights}

    def predict_and_render_chunk(self, ray_chunks, u=None, seed=0, ray_offset=0):
        """nerf.py:218-227"""
        out = self._ctx.render_chunk(*ray_chunks, u=u, seed=seed, ray_offset=ray_offset)
        return ({"image": out["c_image"], "depth": out["c_depth"], "weights": out["c_weights"]},
                {"image": out["f_image"], "depth": out["f_depth"], "weights": out["f_weights"]})

    # ------------------------------------------------------------------ the trained field (extension, no reference counterpart)
    def _field_net(self, net) -> int:
        if self._ctx is None:
            raise RuntimeError("the model is not compiled: call compile(...) before query / density_grid / extract_mesh")
        if net not in ("coarse", "fine"):
            raise ValueError(f"net must be 'coarse' or 'fine', got {net!r}")
        return COARSE if net == "coarse" else FINE

    @staticmethod
    def _grid_spec(resolution, bounds):
        res = (resolution,) * 3 if isinstance(resolution, (int, np.integer)) else tuple(resolution)
        if len(res) != 3 or any(int(r) != r or int(r) < 2 for r in res):
            raise ValueError(f"resolution must be an int or three ints, each >= 2; got {resolution!r}")
        lo, hi = (tuple(float(v) for v in b) for b in bounds)
        if len(lo) != 3 or len(hi) != 3 or not all(np.float32(h) > np.float32(l) for l, h in zip(lo, hi)):
            raise ValueError(f"bounds must be (lo[3], hi[3]) with hi > lo on every axis; got {bounds!r}")
        return tuple(int(r) for r in res), lo, hi

    def query(self, points, directions=None, net="fine"):
        """The trained MLP at points [..., 3] (any leading shape), viewed along directions None (zero vector), [3] or [..., 3]:
        (rgb [..., 3] after sigmoid, sigma [..., 1] after relu) -- NeRFMLP.__call__'s contract on raw coordinates.  Fused shapes
        run one fused kernel (the render path's encoding, trunk and head, bit for bit)."""
        n = self._field_net(net)
        p = self._ctx.f32(points)
        if p.dim() < 1 or p.shape[-1] != 3:
            raise ValueError(f"points must have a last dimension of 3, got {tuple(p.shape)}")
        lead = tuple(p.shape[:-1])
        d = None
        if directions is not None:
            d = self._ctx.f32(directions)
            if d.shape[-1] != 3:
                raise ValueError(f"directions must have a last dimension of 3, got {tuple(d.shape)}")
            if d.numel() != 3:
                d = torch.broadcast_to(d, p.shape).contiguous()
        sigma, rgb = self._ctx.query_points(n, p.reshape(-1, 3), None if d is None else d.reshape(-1, 3), raw=False, rgb=True)
        return rgb.reshape(lead + (3,)), sigma.reshape(lead + (1,))

    def density_grid(self, resolution, bounds=((-1.5,) * 3, (1.5,) * 3), net="fine", direction=None):
        """sigma [Rx, Ry, Rz] of the trained MLP on the grid lo + idx * (hi - lo) / (R - 1) (C order, z fastest); resolution an int
        or a 3-tuple.  With `direction` ([3]): (sigma, rgb [Rx, Ry, Rz, 3]) seen along it."""
        n = self._field_net(net)
        res, lo, hi = self._grid_spec(resolution, bounds)
        sigma, rgb = self._ctx.query_grid(n, res, lo, hi, direction, rgb=direction is not None)
        return sigma if direction is None else (sigma, rgb)

    def extract_mesh(self, threshold, resolution=256, bounds=((-1.5,) * 3, (1.5,) * 3), net="fine", vertex_colors=False):
        """Marching cubes on density_grid(resolution, bounds, net) at sigma = threshold (inside: sigma > threshold): (vertices [V,3]
        f32, faces [F,3] int32, normals [V,3]), torch tensors on the model's device; normals point outward (toward lower density).
        vertex_colors: also rgb [V,3] queried at each vertex along -normal.  An empty surface gives empty arrays.
        keras_nerf_amd.io.ply.save_ply writes the result."""
        res, lo, hi = self._grid_spec(resolution, bounds)
        sigma = self.density_grid(res, (lo, hi), net)
        verts, faces, normals = marching_cubes(sigma, float(threshold), lo, hi)
        if not vertex_colors:
            return verts, faces, normals
        colors = self.query(verts, -normals, net)[0]
        return verts, faces, normals, colors

    def bake(self, resolution=256, bounds=((-1.5,) * 3, (1.5,) * 3), net="fine", sh_degree=2, n_directions=None, sigma_threshold=0.0,
             bricks=None, quantize=False):
        """Bake the trained field into a keras_nerf_amd.baked.BakedField: density_grid(resolution, bounds, net) with every value
        <= sigma_threshold stored as 0, and at every lattice point that touches an occupied cell the colour as a function of the view
        direction, fitted by least squares with real spherical harmonics up to sh_degree (0..3) from the net's colour along
        n_directions Fibonacci-sphere directions (default max(4 K, 16), K = (sh_degree + 1)^2; sh_degree 0: the single zero
        direction).  sigma_threshold must be >= 0.  The fit runs over slabs of the lattice, with about 1 GB of working memory whatever
        the resolution.  BakedField.render then renders novel views from the grid alone, without the MLP.
        bricks = 4 or 8 (default None: the dense BakedField, as ever): bake straight into a keras_nerf_amd.baked.BrickBakedField that
        stores only the bricks of bricks^3 lattice points around occupied cells; the dense record table is never allocated and the
        result is bake(...).compact(bricks) byte for byte.
        quantize=True (default False; needs bricks, ValueError otherwise): the keras_nerf_amd.baked_quant.QuantizedBrickField
        bake(bricks=bricks).quantize(), byte for byte -- SH coefficients as 8-bit values with a scale per brick and SH band, records
        of half the size.  The unquantised brick field exists transiently while the result is formed."""
        from ...baked import bake
        return bake(self, resolution, bounds, net, sh_degree, n_directions, sigma_threshold, bricks=bricks, quantize=quantize)

    # ------------------------------------------------------------------ empty-space skipping for rendering (extension)
    def build_occupancy_grid(self, resolution=128, bounds=((-1.5,) * 3, (1.5,) * 3), threshold=0.0, dilation=1, outside="occupied"):
        """An occupancy grid for each net from its own density_grid(resolution + 1, bounds): a cell is occupied if one of its 8 corners
        has sigma > threshold, then dilated by `dilation` cells (0..8).  Both grids are attached (set_occupancy_grid) and returned as
        {"coarse": bool [cx, cy, cz], "fine": ...} NumPy arrays.  From then on every render (predict_and_render_images,
        predict_and_render_chunk, test_step / evaluate) runs each MLP only on samples in its occupied cells; training never skips.
        A heuristic: density between lattice points can be missed, the dilation is the margin.  The grids hold the weights as they
        are now (training does not update them) and are not saved by save_model."""
        cells = (resolution,) * 3 if isinstance(resolution, (int, np.integer)) else \
            (tuple(resolution) if isinstance(resolution, (tuple, list)) else ())
        if len(cells) != 3 or any(isinstance(c, bool) or int(c) != c or not 1 <= int(c) <= 1024 for c in cells):
            raise ValueError(f"resolution must be an int or three ints, each 1..1024 cells; got {resolution!r}")
        if outside not in OCCUPANCY_OUTSIDE:
            raise ValueError(f"outside must be 'occupied' or 'empty', got {outside!r}")
        if isinstance(dilation, bool) or not isinstance(dilation, (int, np.integer)) or not 0 <= dilation <= 8:
            raise ValueError(f"dilation must be an integer 0..8, got {dilation!r}")
        if not np.isfinite(float(threshold)):
            raise ValueError(f"threshold must be finite, got {threshold!r}")
        res, lo, hi = self._grid_spec(tuple(int(c) + 1 for c in cells), bounds)
        self._field_net("fine")
        grids = {}
        for name in ("coarse", "fine"):
            grids[name] = occupancy_from_grid(self.density_grid(res, (lo, hi), name), float(threshold), int(dilation))
        for name in ("coarse", "fine"):
            self.set_occupancy_grid(name, grids[name], (lo, hi), outside=outside)
        return grids

    def set_occupancy_grid(self, net, occupied, bounds=((-1.5,) * 3, (1.5,) * 3), outside="occupied"):
        """Attach a boolean occupancy grid [cx, cy, cz] (1..1024 cells per axis) over bounds = (lo[3], hi[3]) to net "coarse" or
        "fine"; None detaches it.  outside: "occupied" or "empty" for samples outside the box (include/knerf.h knerf_set_occupancy)."""
        if occupied is not None:
            try:
                lo, hi = bounds
            except (TypeError, ValueError):
                raise ValueError(f"bounds must be (lo[3], hi[3]); got {bounds!r}") from None
            occupancy_spec(occupied, lo, hi, outside)            # ValueError on a bad grid, box or policy (before the compile check)
        n = self._field_net(net)
        if occupied is None:
            self._ctx.set_occupancy(n, None)
        else:
            self._ctx.set_occupancy(n, occupied, lo, hi, outside)

    def clear_occupancy_grid(self):
        """Detach both nets' grids: renders are dense again"""
        for name in ("coarse", "fine"):
            self.set_occupancy_grid(name, None)

    def occupancy_stats(self, reset=True):
        """{"coarse": (live, total), "fine": (live, total)}: samples of the render passes in occupied cells / samples those passes
        considered, since the last reset"""
        self._field_net("fine")
        c, f = self._ctx.occupancy_stats(reset)
        return {"coarse": c, "fine": f}

    def set_occupancy_training(self, on):
        """Train behind the attached grids (option occupancy_train, include/knerf.h): with on=True every train pass of a net that has
        a grid treats the samples in its empty cells as renders do (raw = 0, the MLP not evaluated there, no gradient from them); nets
        without a grid train as before.  False: training is dense again (the grids stay attached for renders).  OccupancyGridUpdater
        (callback.py) builds the grids during fit and turns this on."""
        if not isinstance(on, (bool, np.bool_)) and on not in (0, 1):
            raise ValueError(f"set_occupancy_training: on must be True / False (or 1 / 0), got {on!r}")
        self._field_net("fine")
        self._ctx.set_option("occupancy_train", int(bool(on)))

    def occupancy_train_stats(self, reset=True):
        """{"coarse": (live, total), "fine": (live, total)}: samples of the TRAIN passes behind a grid whose MLP was evaluated /
        samples those passes considered, since the last reset (renders are counted by occupancy_stats)"""
        self._field_net("fine")
        c, f = self._ctx.occupancy_train_stats(reset)
        return {"coarse": c, "fine": f}

    # ------------------------------------------------------------------ early ray termination for rendering (extension)
    def set_ray_termination(self, threshold=1e-4, segment=None):
        """Early ray termination of every render (options termination_threshold / termination_segment, include/knerf.h): each render
        pass works in segments of `segment` samples (1..1024; None keeps the current length, 32 by default), and once a ray's
        transmittance T has dropped below `threshold` in front of a segment, the MLP no longer runs on that segment and the ones behind
        it (raw = 0 there).  Samples in front of the cut keep their exact values; per ray the image moves by at most `threshold` and the
        depth by at most threshold * far.  threshold = 0 turns it off: renders are then bit-identical to renders without it.  While it
        is on, predict_and_render_images, predict_and_render_chunk, test_step and evaluate are affected; training never terminates."""
        if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)) or \
                not np.isfinite(float(threshold)) or not 0.0 <= float(threshold) < 1.0:
            raise ValueError(f"threshold must be a finite number in [0, 1), got {threshold!r}")
        if segment is not None and (isinstance(segment, (bool, np.bool_)) or not isinstance(segment, (int, np.integer)) or
                                    not 1 <= int(segment) <= 1024):
            raise ValueError(f"segment must be None or an integer 1..1024, got {segment!r}")
        self._field_net("fine")
        if segment is not None:
            self._ctx.set_option("termination_segment", int(segment))
        self._ctx.set_option("termination_threshold", float(threshold))

    def termination_stats(self, reset=True):
        """{"coarse": (evaluated, total), "fine": (evaluated, total)}: samples of the render passes with early ray termination on whose
        MLP output was kept (occupied, when a grid is attached, and not terminated) / every sample of those passes, since the last reset"""
        self._field_net("fine")
        c, f = self._ctx.termination_stats(reset)
        return {"coarse": c, "fine": f}

    def predict_and_render_images(self, rays, u=None, outputs=None):
        """nerf.py:229-304: returns (coarse_results, fine_results), each {image [B,H,W,3], depth [B,H,W], weights [B,H,W,S]}.
        outputs (extension): the keys wanted, e.g. ("image", "depth") -- what inference.py:108-114 reads -- or ("image",) (test_step);
        the others are neither allocated nor written (knerf_render_batch takes NULL for them: at 256 x 256 the two `weights` arrays
        are 67 MB per frame).  Default: the reference's full dictionaries.  Behind an occupancy grid (build_occupancy_grid) or with early
        ray termination on (set_ray_termination) the MLPs skip samples, and the outputs follow include/knerf.h."""
        keys = ("image", "depth", "weights") if outputs is None else tuple(outputs)
        if "image" not in keys or any(k not in ("image", "depth", "weights") for k in keys):
            raise ValueError("outputs must contain 'image' and may contain 'depth' and 'weights'")
        o, d, t = self._flat_rays(rays)
        N, R, Nc, Na = self.num_rays, self.ray_chunks, self.n_coarse, self.n_coarse + self.n_fine
        e = lambda *s: torch.empty(s, device=self.device)
        buf = dict(c_image=e(N, 3), f_image=e(N, 3))
        if "depth" in keys:
            buf.update(c_depth=e(N), f_depth=e(N))
        if "weights" in keys:
            buf.update(c_weights=e(N, Nc), f_weights=e(N, Na))
        uf = None if u is None else self._ctx.f32(u).reshape(N, self.n_fine)
        seed = self._next_seed()
        # the chunk loop of nerf.py:236-288 runs inside the library: one host call per batch of images
        self._ctx.render_batch(o, d, t, uf, seed, R, out=buf)
        B, H, W = self.batch_size, self.image_height, self.image_width
        shape = {"image": (B, H, W, 3), "depth": (B, H, W)}
        coarse = {k: buf["c_" + k].reshape(shape.get(k, (B, H, W, Nc))) for k in keys}
        fine = {k: buf["f_" + k].reshape(shape.get(k, (B, H, W, Na))) for k in keys}
        return coarse, fine

    call = predict_and_render_images          # the reference defines no call(); Keras users expect one
    __call__ = predict_and_render_images

    # ------------------------------------------------------------------ metrics (nerf.py:306-330)
    def update_and_return_metrics(self, images, coarse_images, fine_images, coarse_loss, fine_loss):
        """two metric launches (each yields both the SSIM and the squared-error sums of one image pair) + one update of the
        device-side means; returns the six running means as a mapping that reads them back lazily (metrics.MetricLogs)"""
        losses = torch.stack([torch.as_tensor(coarse_loss, device=self.device).reshape(()).float(),
                              torch.as_tensor(fine_loss, device=self.device).reshape(()).float()])
        self._metric_state.update(images, coarse_images, fine_images, losses)
        return self._metric_state.snapshot()

    # ------------------------------------------------------------------ train / test step
    def train_step(self, inputs, u=None, with_metrics=True, sync=True):
        """nerf.py:332-473.  inputs = (images [B,H,W,3|4], (o, d, t)).  Returns the six running means (read back lazily).
        A 2-D first element makes it a step on scattered rays (data.RayBatchDataset): inputs = (target [n,3], (o [n,3], d [n,3],
        t [n,n_coarse])) with n a multiple of ray_chunks; its logs carry the losses and PSNRs, no SSIM.
        sync=True (a direct call): waits for the step, so a non-finite gradient raises from THIS call as in the reference
        (nerf.py:381-382).  sync=False (what `fit` uses): nothing waits for the GPU; a skipped step raises from the first later
        poll (fit polls at every epoch end, save_model and get_weights poll before they read weights)."""
        images, rays = inputs
        ray_mode = getattr(images, "ndim", None) == 2          # a batch of scattered rays: (target [n,3], (o [n,3], d [n,3], t [n,Nc]))
        if ray_mode:
            tgt = self._ctx.f32(images)[:, :3].contiguous()
            N, R = tgt.shape[0], self.ray_chunks
            if N % R:
                raise ValueError(f"a batch of {N} rays is not a multiple of ray_chunks = {R}")
            f = self._ctx.f32
            o, d, t = f(rays[0]).reshape(N, 3), f(rays[1]).reshape(N, 3), f(rays[2]).reshape(N, self.n_coarse)
        else:
            images = self._ctx.f32(images)[..., :3].contiguous()                  # nerf.py:335
            o, d, t = self._flat_rays(rays)
            N, R = self.num_rays, self.ray_chunks
            tgt = images.reshape(N, 3)
        uf = None if u is None else self._ctx.f32(u).reshape(N, self.n_fine)
        ci = torch.empty((N, 3), device=self.device); fi = torch.empty((N, 3), device=self.device)
        self._loss_acc.zero_()
        seed = self._next_seed()
        # the chunk loop of nerf.py:351-421 (C chunks of R rays, gradients and losses accumulated with weight 1/C) runs
        # inside the library: one host call per step
        self._ctx.train_batch(o, d, t, tgt, uf, seed, R, self._loss_acc, ci, fi)
        if self._dist:                                                            # nerf.py:455-458 under MirroredStrategy
            timing = getattr(self, "_allreduce_events", None)                     # bench.py: events around the collective
            if timing is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            parallel.all_reduce_gradients(self._ctx.grads_view(), self.all_reduce)
            if timing is not None:
                e1.record(); timing.append((e0, e1))
        # finite check (nerf.py:381-382), 2x Adam, accumulators zeroed (nerf.py:464-471): enqueued, nothing waits for the GPU
        self._ctx.apply_adam(check=False)
        if self.run_eagerly:
            self._zero_gradient_diagnostics(wait=bool(sync))
        if not with_metrics:
            # fast path (no host synchronisation per step): a step skipped for a non-finite gradient is reported by the
            # first later call that finds it completed
            self._ctx.poll_nonfinite(wait=False)
            return {"coarse_loss": self._loss_acc[0], "fine_loss": self._loss_acc[1]}
        if ray_mode:
            # the chunks are equally sized, so the accumulated losses are the batch's mean squared errors: losses and PSNR, no SSIM
            # (another objective: the PSNR stays a PSNR -- it comes from the squared-error terms the kernel accumulates beside the loss)
            self._metric_state.update_rays(self._loss_acc, None if self._objective_plain else self._ctx.objective_terms()[:, 1])
            logs = self._metric_state.snapshot(RAY_NAMES)
        else:
            B, H, W = self.batch_size, self.image_height, self.image_width
            self._metric_state.update(images, ci.reshape(B, H, W, 3), fi.reshape(B, H, W, 3), self._loss_acc)
            logs = self._metric_state.snapshot()
        self._ctx.poll_nonfinite(wait=bool(sync))      # sync: as the reference, the failing batch raises from its own train_step
        return logs

    def test_step(self, inputs, u=None):
        """nerf.py:475-497 (renders through predict_and_render_images: behind the occupancy grids and with early ray termination
        when those are on)"""
        images, rays = inputs
        images = self._ctx.f32(images)[..., :3].contiguous()
        coarse, fine = self.predict_and_render_images(rays, u, outputs=("image",))     # nerf.py:489-497 reads the two images only
        # whole-image MSE (nerf.py:484-487) from the metrics kernel's squared-difference sums (losses=None)
        losses = None
        if self._objective.loss_kind != 0:
            # the chosen photometric term of the two images, without regularisers (one torch reduction each; not the hot path)
            losses = torch.stack([self._loss_fn(images, coarse["image"]), self._loss_fn(images, fine["image"])]).float()
        self._metric_state.update(images, coarse["image"], fine["image"], losses)
        return self._metric_state.snapshot()

    def objective_terms(self):
        """The terms of the last train step's objective, {"coarse": {...}, "fine": {...}} with photometric (the chosen loss), mse,
        distortion and opacity_entropy (the means over rays of D and H, unweighted) and total (= the net's logged loss).  Lazy: the
        values leave the device when first read.  Under plain mean squared error the kernel computes no terms and all are 0."""
        if self._ctx is None:
            raise RuntimeError("the model is not compiled: call compile(...) first")
        return ObjectiveTerms(self._ctx.objective_terms(), self._objective)

    def evaluate(self, dataset, return_dict=False, callbacks=None, verbose=0):
        """tf.keras.Model.evaluate on the reference's test_step (nerf.py:475-497): the metrics averaged over the dataset's batches, as
        a list in `metrics_names` order or as a dict (data-parallel: the replicas' mean, as fit's validation logs)."""
        callbacks = list(callbacks or [])
        for cb in callbacks:
            getattr(cb, "on_test_begin", lambda logs=None: None)({})
        self.reset_metrics()
        logs = {}
        for b, batch in enumerate(dataset):
            logs = self.test_step(batch)
            for cb in callbacks:
                getattr(cb, "on_test_batch_end", lambda i, logs=None: None)(b, logs)
        logs = parallel.reduce_logs({k: float(v) for k, v in dict(logs).items()}, self.device)
        for cb in callbacks:
            getattr(cb, "on_test_end", lambda logs=None: None)(dict(logs))
        if verbose:
            logging.info("evaluate - %s", " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()))
        return logs if return_dict else [logs[k] for k in self.metrics_names if k in logs]

    # ------------------------------------------------------------------ fit: the part of tf.keras.Model.fit the reference uses
    def fit(self, dataset, epochs=1, validation_data=None, callbacks=None, initial_epoch=0, verbose=1):
        """train_single.py:137-143.  dataset yields (images, (o, d, t)) batches and is re-iterable; callbacks get the Keras
        hooks NeRFTrainMonitor uses (set_model, on_train_batch_end, on_epoch_end).  Returns a Keras-style History ({key: [per-epoch
        values]} as `.history`, and as the object itself)."""
        callbacks = list(callbacks or [])
        for cb in callbacks:
            if hasattr(cb, "set_model"):
                cb.set_model(self)
            else:
                cb.model = self
        history: Dict[str, list] = {}
        epochs_run = []
        self.stop_training = False
        for cb in callbacks:
            getattr(cb, "on_train_begin", lambda logs=None: None)({})
        for epoch in range(initial_epoch, epochs):
            self.reset_metrics()
            for cb in callbacks:
                getattr(cb, "on_epoch_begin", lambda e, logs=None: None)(epoch, {})
            logs = {}
            for b, batch in enumerate(dataset):
                # asynchronous: the step is enqueued, its logs stay on the device until a callback reads them (MetricLogs)
                logs = self.train_step(batch, sync=False)
                for cb in callbacks:
                    getattr(cb, "on_train_batch_end", lambda i, logs=None: None)(b, logs)
            logs = {k: float(v) for k, v in dict(logs).items()}            # one read-back per epoch
            self._ctx.poll_nonfinite(wait=True)                            # a skipped step of this epoch raises here at the latest
            if validation_data is not None:
                for cb in callbacks:
                    getattr(cb, "on_test_begin", lambda logs=None: None)({})
                self.reset_metrics()
                vlogs = {}
                for batch in validation_data:
                    vlogs = self.test_step(batch)
                logs.update({"val_" + k: float(v) for k, v in dict(vlogs).items()})
                for cb in callbacks:
                    getattr(cb, "on_test_end", lambda logs=None: None)(dict(logs))
            logs = parallel.reduce_logs(logs, self.device)    # replica means (one tiny all-reduce)
            for k, v in logs.items():
                history.setdefault(k, []).append(v)
            epochs_run.append(epoch)
            if verbose:
                logging.info("Epoch %d/%d - %s", epoch + 1, epochs, " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()))
            for cb in callbacks:
                getattr(cb, "on_epoch_end", lambda e, logs=None: None)(epoch, logs)
            if self.stop_training:
                break
        for cb in callbacks:
            getattr(cb, "on_train_end", lambda logs=None: None)({})
        try:
            steps = len(dataset)
        except TypeError:
            steps = None
        self.history = History(history, epochs_run, {"epochs": epochs, "steps": steps, "verbose": verbose})
        return self.history


class ObjectiveTerms(dict):
    """NeRF.objective_terms(): a dict of two dicts whose numbers are read back from the device on first access"""

    _KEYS = ("photometric", "mse", "distortion", "opacity_entropy")

    def __init__(self, dev, objective):
        super().__init__()
        self._dev, self._obj = dev, objective

    def _fill(self):
        if self._dev is not None:
            v, o = self._dev.cpu().numpy().astype(np.float64), self._obj
            self._dev = None
            for n, name in enumerate(("coarse", "fine")):
                d = dict(zip(self._KEYS, (float(x) for x in v[n])))
                on = (o.nets >> n) & 1
                d["total"] = d["photometric"] + (o.distortion * d["distortion"] + o.opacity_entropy * d["opacity_entropy"] if on else 0.0)
                dict.__setitem__(self, name, d)

    def __getitem__(self, k):
        self._fill()
        return dict.__getitem__(self, k)

    def __iter__(self):
        self._fill()
        return dict.__iter__(self)

    def __len__(self):
        return 2

    def keys(self):
        self._fill()
        return dict.keys(self)

    def items(self):
        self._fill()
        return dict.items(self)

    def values(self):
        self._fill()
        return dict.values(self)

    def __repr__(self):
        self._fill()
        return dict.__repr__(self)

