"""Optimizer configuration under the Keras names: `Adam` and the three learning-rate schedules `NeRF.compile(optimizer=...)` accepts
beside the string 'adam' (the reference hands its argument to tf.keras.optimizers.get, keras_nerf/model/nerf/nerf.py:163-165).

These classes HOLD a configuration: `get_config()` in the Keras serialised form, and for a schedule `__call__(step)` in Python floats.
They compute nothing else -- the update runs in csrc/optim.hip / csrc/optim_ext.hip behind knerf_set_optimizer (include/knerf.h) --
and they are no alias of any TensorFlow module: a real tf.keras optimizer object, or its serialised dict, is accepted by `compile`
just the same, through its own `get_config()`.

`OptimizerSpec` is the normal form all of them are parsed into (model/nerf/nerf.py `_optimizer_spec`): what the C ABI's
knerf_optimizer struct holds plus Adam's beta_1, beta_2 and epsilon."""
from __future__ import annotations

import json
import math
import os
import types
from typing import Optional

import numpy as np

from . import _lib

MAX_VALUES = _lib.SCHEDULE_MAX_VALUES


def _number(name, v, positive=False):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name}={v!r} is not a number")
    v = float(v)
    if not math.isfinite(v) or v < 0 or (positive and v == 0):
        raise ValueError(f"{name}={v!r} must be finite and {'> 0' if positive else '>= 0'}")
    return v


class LearningRateSchedule:
    """base of the three schedules; step = the number of optimizer steps applied so far (Keras' `iterations`)"""

    def get_config(self):
        raise NotImplementedError

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def __call__(self, step):
        raise NotImplementedError


class ExponentialDecay(LearningRateSchedule):
    """initial_learning_rate * decay_rate ** (step / decay_steps); staircase: the exponent is floored"""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate = _number("ExponentialDecay initial_learning_rate", initial_learning_rate)
        self.decay_steps = _number("ExponentialDecay decay_steps", decay_steps, positive=True)
        self.decay_rate = _number("ExponentialDecay decay_rate", decay_rate)
        self.staircase = bool(staircase)
        self.name = name

    def __call__(self, step):
        p = float(step) / self.decay_steps
        if self.staircase:
            p = math.floor(p)
        return self.initial_learning_rate * self.decay_rate ** p

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps, "decay_rate": self.decay_rate,
                "staircase": self.staircase, "name": self.name}


class CosineDecay(LearningRateSchedule):
    """s = min(step, decay_steps); initial_learning_rate * ((1 - alpha) * 0.5 * (1 + cos(pi s / decay_steps)) + alpha).  The warm-up
    variant of Keras 3 (warmup_target / warmup_steps) is not implemented and is refused."""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name=None, warmup_target=None, warmup_steps=0):
        if warmup_target is not None or warmup_steps not in (None, 0):
            raise ValueError("CosineDecay warmup_target / warmup_steps: the warm-up variant is not implemented")
        self.initial_learning_rate = _number("CosineDecay initial_learning_rate", initial_learning_rate)
        self.decay_steps = _number("CosineDecay decay_steps", decay_steps, positive=True)
        self.alpha = _number("CosineDecay alpha", alpha)
        self.name = name

    def __call__(self, step):
        s = min(float(step), self.decay_steps)
        return self.initial_learning_rate * ((1.0 - self.alpha) * (0.5 * (1.0 + math.cos(math.pi * s / self.decay_steps))) + self.alpha)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps, "alpha": self.alpha,
                "name": self.name}


class PiecewiseConstantDecay(LearningRateSchedule):
    """values[i] for the first i with step <= boundaries[i], else the last value; len(values) == len(boundaries) + 1 <= 16"""

    def __init__(self, boundaries, values, name=None):
        b, v = list(boundaries), list(values)
        if len(v) != len(b) + 1:
            raise ValueError(f"PiecewiseConstantDecay: {len(b)} boundaries need {len(b) + 1} values, got {len(v)}")
        if len(v) > MAX_VALUES:
            raise ValueError(f"PiecewiseConstantDecay: at most {MAX_VALUES} values, got {len(v)}")
        for x in b:
            if isinstance(x, (bool, np.bool_)) or float(x) != int(x) or int(x) < 0:
                raise ValueError(f"PiecewiseConstantDecay boundaries must be integers >= 0, got {x!r}")
        self.boundaries = [int(x) for x in b]
        if any(y <= x for x, y in zip(self.boundaries, self.boundaries[1:])):
            raise ValueError(f"PiecewiseConstantDecay boundaries must ascend, got {self.boundaries}")
        self.values = [_number("PiecewiseConstantDecay value", x) for x in v]
        self.name = name

    def __call__(self, step):
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]

    def get_config(self):
        return {"boundaries": list(self.boundaries), "values": list(self.values), "name": self.name}


SCHEDULE_CLASSES = {"ExponentialDecay": ExponentialDecay, "CosineDecay": CosineDecay, "PiecewiseConstantDecay": PiecewiseConstantDecay}
schedules = types.SimpleNamespace(LearningRateSchedule=LearningRateSchedule, **SCHEDULE_CLASSES)


def serialize_schedule(s: LearningRateSchedule) -> dict:
    return {"class_name": type(s).__name__, "config": s.get_config()}


def schedule_from(value, what="learning_rate") -> LearningRateSchedule:
    """one of the three schedules from one of them, from any object of such a class NAME with a get_config() (a tf.keras schedule) or
    from the serialised form {"class_name", "config"}; ValueError naming `what` for everything else (unknown classes, callables)"""
    if isinstance(value, LearningRateSchedule):
        return value
    if isinstance(value, dict):
        if "class_name" not in value or not isinstance(value.get("config"), dict):
            raise ValueError(f"Adam {what}: a dict must be the serialised form {{'class_name', 'config'}} of a schedule, got {value!r}")
        name, cfg = str(value["class_name"]), dict(value["config"])
    elif callable(getattr(value, "get_config", None)):
        name, cfg = type(value).__name__, dict(value.get_config())
    else:
        raise ValueError(f"Adam {what}={value!r}: a number or one of the schedules {sorted(SCHEDULE_CLASSES)} is implemented "
                         f"(a plain callable is not)")
    cls = SCHEDULE_CLASSES.get(name.rsplit(">", 1)[-1].rsplit(".", 1)[-1])
    if cls is None:
        raise ValueError(f"Adam {what}: learning-rate schedule {name} is not implemented (only {sorted(SCHEDULE_CLASSES)})")
    try:
        return cls(**cfg)
    except TypeError as e:
        raise ValueError(f"Adam {what}: {name} does not take this configuration ({e})") from None


class Adam:
    """tf.keras.optimizers.Adam's argument names and defaults.  amsgrad and use_ema are held so that `compile` can refuse them by name."""

    def __init__(self, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, weight_decay=None, clipnorm=None,
                 clipvalue=None, global_clipnorm=None, use_ema=False, name="adam", **kwargs):
        if kwargs:
            raise ValueError(f"Adam: unknown argument(s) {sorted(kwargs)}")
        self.learning_rate = learning_rate
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        self.amsgrad, self.use_ema = bool(amsgrad), bool(use_ema)
        self.weight_decay, self.clipnorm, self.clipvalue, self.global_clipnorm = weight_decay, clipnorm, clipvalue, global_clipnorm
        self.name = name

    def get_config(self):
        lr = self.learning_rate
        if isinstance(lr, LearningRateSchedule):
            lr = serialize_schedule(lr)
        elif callable(getattr(lr, "get_config", None)):
            lr = {"class_name": type(lr).__name__, "config": dict(lr.get_config())}
        return {"name": self.name, "learning_rate": lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon,
                "amsgrad": self.amsgrad, "weight_decay": self.weight_decay, "clipnorm": self.clipnorm, "clipvalue": self.clipvalue,
                "global_clipnorm": self.global_clipnorm, "use_ema": self.use_ema}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


CLIP_KINDS = {"clipvalue": _lib.CLIP_VALUE, "clipnorm": _lib.CLIP_NORM, "global_clipnorm": _lib.CLIP_GLOBAL_NORM}


class OptimizerSpec:
    """The parsed optimizer: Adam's four numbers, the schedule (None: the constant rate `lr`), at most one clip option
    (clip = "clipvalue" | "clipnorm" | "global_clipnorm" or None, with clip_arg) and the decoupled weight decay."""

    def __init__(self, lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7, schedule: Optional[LearningRateSchedule] = None, clip=None,
                 clip_arg=0.0, weight_decay=0.0):
        if schedule is not None and not isinstance(schedule, LearningRateSchedule):
            schedule = schedule_from(schedule)
        if clip is not None and clip not in CLIP_KINDS:
            raise ValueError(f"clip must be one of {sorted(CLIP_KINDS)} or None, got {clip!r}")
        self.lr = _number("Adam learning_rate", lr) if schedule is None else float(schedule(0))
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.schedule = schedule
        self.clip = clip
        self.clip_arg = _number(f"Adam {clip}", clip_arg, positive=True) if clip is not None else 0.0
        self.weight_decay = _number("Adam weight_decay", 0.0 if weight_decay is None else weight_decay)

    @property
    def is_plain(self) -> bool:
        """plain Adam with a constant rate: the kernels of csrc/optim.hip, nothing of csrc/optim_ext.hip"""
        return self.schedule is None and self.clip is None and self.weight_decay == 0.0

    def lr_at(self, step: int) -> float:
        return self.lr if self.schedule is None else float(self.schedule(int(step)))

    def to_struct(self) -> "_lib.KnerfOptimizer":
        o = _lib.KnerfOptimizer()
        s = self.schedule
        o.lr = self.lr
        if isinstance(s, ExponentialDecay):
            o.schedule, o.lr, o.decay_steps, o.decay_rate, o.staircase = _lib.SCHEDULE_EXPONENTIAL, s.initial_learning_rate, s.decay_steps, s.decay_rate, int(s.staircase)
        elif isinstance(s, CosineDecay):
            o.schedule, o.lr, o.decay_steps, o.alpha = _lib.SCHEDULE_COSINE, s.initial_learning_rate, s.decay_steps, s.alpha
        elif isinstance(s, PiecewiseConstantDecay):
            o.schedule, o.n_values, o.lr = _lib.SCHEDULE_PIECEWISE, len(s.values), 0.0
            for i, b in enumerate(s.boundaries):
                o.boundaries[i] = b
            for i, v in enumerate(s.values):
                o.values[i] = v
        elif s is not None:
            raise ValueError(f"schedule {type(s).__name__} is not implemented")
        if self.clip is not None:
            o.clip, o.clip_arg = CLIP_KINDS[self.clip], self.clip_arg
        o.weight_decay = self.weight_decay
        return o

    def get_config(self) -> dict:
        """the Keras serialised form {"class_name": "Adam", "config": {...}} (JSON-able; `compile` takes it back)"""
        cfg = {"name": "adam", "learning_rate": self.lr if self.schedule is None else serialize_schedule(self.schedule),
               "beta_1": self.beta1, "beta_2": self.beta2, "epsilon": self.epsilon, "amsgrad": False,
               "weight_decay": self.weight_decay or None, "clipnorm": None, "clipvalue": None, "global_clipnorm": None, "use_ema": False}
        if self.clip is not None:
            cfg[self.clip] = self.clip_arg
        return {"class_name": "Adam", "config": cfg}


# ---- optimizer_state.npz (NeRF.save_model(optimizer_state=True) / NeRF.load_optimizer_state) ---------------------------------------
STATE_FILE = "optimizer_state.npz"
_STATE_KEYS = ("coarse_m", "coarse_v", "fine_m", "fine_v")


def save_optimizer_state(path: str, step: int, slots: dict, config: dict) -> str:
    """writes <path>/optimizer_state.npz: the count of applied steps, Adam's m and v of both nets as flat float32 vectors at their
    REAL widths (slots: {"coarse_m", "coarse_v", "fine_m", "fine_v"}) and the optimizer configuration (JSON)"""
    arrays = {}
    for k in _STATE_KEYS:
        arrays[k] = np.ascontiguousarray(np.asarray(slots[k], dtype=np.float32).reshape(-1))
    sizes = {a.size for a in arrays.values()}
    if len(sizes) != 1:
        raise ValueError(f"optimizer state: the four slot vectors differ in size {sorted(sizes)}")
    os.makedirs(path, exist_ok=True)
    file = os.path.join(path, STATE_FILE)
    with open(file, "wb") as f:
        np.savez(f, step=np.int64(step), config=np.array(json.dumps(config)), **arrays)
    return file


def load_optimizer_state(path: str):
    """(step, slots, config) as save_optimizer_state wrote them; `path` is the model directory or the file itself"""
    file = os.path.join(path, STATE_FILE) if os.path.isdir(path) else path
    with np.load(file, allow_pickle=False) as z:
        missing = [k for k in ("step", "config") + _STATE_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{file}: not an optimizer state (missing {missing})")
        step = int(z["step"])
        slots = {k: np.ascontiguousarray(z[k], dtype=np.float32) for k in _STATE_KEYS}
        config = json.loads(str(z["config"]))
    if step < 0:
        raise ValueError(f"{file}: negative step count {step}")
    return step, slots, config
