"""The objective of the train step as `NeRF.compile(loss=..., regularizers=...)` takes it: the tf.keras loss classes the fused
compositing kernel implements besides mean squared error, and two regularisers of a ray's weights.

The classes are specifications with the Keras names and `get_config()`; called on two torch tensors they evaluate the same mean in
torch (test_step / evaluate use that; it is not the hot path).  The train step's loss and gradient run in csrc/composite_ext.hip
behind knerf_set_objective (include/knerf.h); plain mean squared error without a regulariser never goes there.

    d = y_pred - y_true, the mean over all elements of
    MeanSquaredError   d^2
    MeanAbsoluteError  |d|
    Huber(delta)       d^2 / 2 where |d| <= delta, else delta (|d| - delta / 2)
    LogCosh            log(cosh(d)) = |d| + log1p(exp(-2 |d|)) - ln 2

    RayRegularizers(distortion, opacity_entropy, nets)
        distortion       weight of the mip-NeRF-360 distortion loss of the ray's weights over the sample intervals
        opacity_entropy  weight of the binary entropy of the ray's accumulated opacity
        nets             "both" | "fine" | "coarse": the nets whose loss carries them
"""
from __future__ import annotations

import math

from . import _lib

_REDUCTIONS_OK = (None, "auto", "sum_over_batch_size", "mean")     # Keras 2 / Keras 3 spellings of the default mean
_NETS = {"coarse": 1, "fine": 2, "both": 3}


class _Loss:
    kind = _lib.LOSS_MSE
    name = "loss"

    def __init__(self, reduction="sum_over_batch_size", name=None):
        _check_reduction(reduction, type(self).__name__)
        self.reduction = reduction
        self.name = name or self.name

    def get_config(self):
        return {"name": self.name, "reduction": self.reduction}

    def rho(self, d):
        raise NotImplementedError

    def __call__(self, y_true, y_pred):
        import torch
        d = torch.as_tensor(y_pred) - torch.as_tensor(y_true)
        return self.rho(d).mean()


class MeanSquaredError(_Loss):
    kind, name = _lib.LOSS_MSE, "mean_squared_error"

    def rho(self, d):
        return d * d


class MeanAbsoluteError(_Loss):
    kind, name = _lib.LOSS_MAE, "mean_absolute_error"

    def rho(self, d):
        return d.abs()


class Huber(_Loss):
    kind, name = _lib.LOSS_HUBER, "huber_loss"

    def __init__(self, delta=1.0, reduction="sum_over_batch_size", name=None):
        super().__init__(reduction, name)
        self.delta = _positive(delta, "Huber delta")

    def get_config(self):
        return dict(super().get_config(), delta=self.delta)

    def rho(self, d):
        import torch
        a = d.abs()
        return torch.where(a <= self.delta, 0.5 * d * d, self.delta * (a - 0.5 * self.delta))


class LogCosh(_Loss):
    kind, name = _lib.LOSS_LOG_COSH, "log_cosh"

    def rho(self, d):
        import torch
        a = d.abs()
        return a + torch.log1p(torch.exp(-2.0 * a)) - math.log(2.0)


class RayRegularizers:
    def __init__(self, distortion=0.0, opacity_entropy=0.0, nets="both"):
        self.distortion = _weight(distortion, "distortion")
        self.opacity_entropy = _weight(opacity_entropy, "opacity_entropy")
        if nets not in _NETS:
            raise ValueError(f"RayRegularizers nets must be 'both', 'fine' or 'coarse', got {nets!r}")
        self.nets = nets

    def get_config(self):
        return {"distortion": self.distortion, "opacity_entropy": self.opacity_entropy, "nets": self.nets}


_BY_NAME = {"mse": MeanSquaredError, "mean_squared_error": MeanSquaredError, "meansquarederror": MeanSquaredError,
            "mae": MeanAbsoluteError, "mean_absolute_error": MeanAbsoluteError, "meanabsoluteerror": MeanAbsoluteError,
            "huber": Huber, "huber_loss": Huber, "log_cosh": LogCosh, "logcosh": LogCosh}


def _check_reduction(reduction, what):
    if reduction not in _REDUCTIONS_OK:
        raise ValueError(f"{what}: reduction={reduction!r} is not implemented (the train step takes the mean over rays and channels)")


def _positive(v, what):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}={v!r} is not a number") from None
    if not (math.isfinite(f) and f > 0):
        raise ValueError(f"{what} must be finite and > 0, got {v!r}")
    return f


def _weight(v, what):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"RayRegularizers {what}={v!r} is not a number") from None
    if not (math.isfinite(f) and f >= 0):
        raise ValueError(f"RayRegularizers {what} must be finite and >= 0, got {v!r}")
    return f


def loss_from(loss) -> _Loss:
    """`loss` as one of this module's classes: a name, one of the classes, an object whose class name and get_config() are those of the
    Keras class (a real tf.keras.losses.Huber), or the serialised {"class_name", "config"} form.  ValueError for anything else -- a
    plain callable cannot run inside the kernel -- and for a reduction other than the default mean."""
    if loss is None:
        return MeanSquaredError()
    if isinstance(loss, _Loss):
        return loss
    if isinstance(loss, str):
        cls = _BY_NAME.get(loss.lower())
        if cls is None:
            raise ValueError(f"loss {loss!r}: the compositing kernel implements mse, mae, huber and log_cosh")
        return cls()
    if isinstance(loss, dict):
        name, cfg = loss.get("class_name"), dict(loss.get("config") or {})
    elif not isinstance(loss, type) and callable(getattr(loss, "get_config", None)):
        name = type(loss).__name__
        try:
            cfg = dict(loss.get_config())
        except Exception:
            cfg = {}
    else:
        raise ValueError(f"loss {loss!r}: a name, a keras_nerf_amd.losses class, a Keras loss object or its serialised form is needed "
                         f"(a plain callable cannot run inside the compositing kernel)")
    cls = _BY_NAME.get(str(name).lower())
    if cls is None:
        raise ValueError(f"loss class {name!r}: the compositing kernel implements MeanSquaredError, MeanAbsoluteError, Huber and LogCosh")
    _check_reduction(cfg.get("reduction", "sum_over_batch_size"), str(name))
    return cls(delta=cfg.get("delta", 1.0)) if cls is Huber else cls()


def regularizers_from(regularizers) -> RayRegularizers:
    if regularizers is None:
        return RayRegularizers()
    if isinstance(regularizers, RayRegularizers):
        return regularizers
    if isinstance(regularizers, dict):
        cfg = dict(regularizers.get("config", regularizers))
        unknown = set(cfg) - {"distortion", "opacity_entropy", "nets"}
        if unknown:
            raise ValueError(f"regularizers: unknown entries {sorted(unknown)}")
        return RayRegularizers(**cfg)
    raise ValueError(f"regularizers {regularizers!r}: a RayRegularizers or its get_config() dict is needed")


def objective_from(loss=None, regularizers=None) -> "_lib.KnerfObjective":
    """the canonical knerf_objective record (include/knerf.h) of a loss and regularisers in any accepted spelling"""
    l, r = loss_from(loss), regularizers_from(regularizers)
    on = r.distortion > 0 or r.opacity_entropy > 0
    return _lib.KnerfObjective(int(l.kind), float(l.delta) if l.kind == _lib.LOSS_HUBER else 0.0, r.distortion, r.opacity_entropy,
                               _NETS[r.nets] if on else 3)


def is_plain(obj: "_lib.KnerfObjective") -> bool:
    """mean squared error without a regulariser: the plain compositing kernel, knerf_set_objective is not needed"""
    return obj.loss_kind == _lib.LOSS_MSE and obj.distortion == 0 and obj.opacity_entropy == 0


def record_tuple(obj: "_lib.KnerfObjective"):
    return (int(obj.loss_kind), float(obj.huber_delta), float(obj.distortion), float(obj.opacity_entropy), int(obj.nets))
