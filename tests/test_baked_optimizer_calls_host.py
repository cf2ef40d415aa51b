"""The launch path of the three baked-field optimisers (BakedFieldOptimizer, BrickFieldOptimizer, BrickGridTrainer) at the level of
ARGUMENTS, without a GPU and without the built library: which entry point an accumulate() reaches and with which values, the order of
the launches of one train_step(), the keys fit() returns, and that every optimiser keyword reaches the optimiser under its own name
through every constructor and factory.

The library is a fake built from _lib.SIGNATURES: every entry point is a ctypes.CFUNCTYPE of the declared types around a Python
callback, so ctypes converts every argument exactly as it would for the real library (a wrong count or type is a ctypes.ArgumentError)
and the callback records the converted values.  Structs passed by reference are read inside the callback, while they exist.

Expected values come from the inputs and from the constants of include/knerf.h as _lib mirrors them."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

from keras_nerf_amd import _lib, baked_bricks_grow, baked_bricks_train, baked_train, losses
from keras_nerf_amd.baked import BakedField, BrickBakedField
from keras_nerf_amd.baked_train import TERM_NAMES, RgbaTargets, check_objective

STRUCTS = {C.POINTER(_lib.KnerfObjective): ("loss_kind", "huber_delta", "distortion", "opacity_entropy"),
           C.POINTER(_lib.KnerfBakedRgba): ("background", "alpha", "stored_background", "opacity")}


class FakeLibrary:
    """getattr gives the entry point of that name as _lib.SIGNATURES declares it; calls: [(name, [converted arguments])], a NULL
    pointer as None, a knerf_objective / knerf_baked_rgba as the dict of its fields, any other struct pointer as True"""

    def __init__(self):
        self.calls, self._functions = [], {}

    def __getattr__(self, name):
        if name.startswith("_") or name not in _lib.SIGNATURES:
            raise AttributeError(name)
        if name not in self._functions:
            restype, argtypes = _lib.SIGNATURES[name]

            def callback(*args):
                seen = []
                for a, t in zip(args, argtypes):
                    if isinstance(a, C._Pointer):
                        a = None if not a else {k: getattr(a.contents, k) for k in STRUCTS[t]} if t in STRUCTS else True
                    seen.append(a)
                self.calls.append((name, seen))
                return 0
            self._functions[name] = C.CFUNCTYPE(restype, *argtypes)(callback)
        return self._functions[name]

    @property
    def names(self):
        return [name for name, _ in self.calls]


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    for module in (baked_train, baked_bricks_train, baked_bricks_grow):
        monkeypatch.setattr(module, "_stream", lambda dev: None)
    return fake


# (class, the stem of its gradient launch, its tv launch or None, its apply launch)
CLASSES = [(baked_train.BakedFieldOptimizer, "knerf_baked_train_rays", "knerf_baked_train_tv", "knerf_baked_train_apply"),
           (baked_bricks_train.BrickFieldOptimizer, "knerf_baked_bricks_train_rays", None, "knerf_baked_bricks_train_apply"),
           (baked_bricks_grow.BrickGridTrainer, "knerf_baked_bricks_train_rays", "knerf_baked_bricks_train_tv",
            "knerf_baked_bricks_train_apply")]
STEP, TERMINATION, LANES, N, N_TOTAL, NEAR = 0.05, 0.01, 2, 5, 7, 0.5
# argument positions of knerf_baked[_bricks]_train_rays[_ext|_rgba] (include/knerf.h)
STREAM, STATE, O, D, NEAR_T, FAR_T, NEAR_ALL, FAR_ALL, TARGET, N_RAYS, N_NORM, H, TERM, FLAGS, SQ, OBJECTIVE, TERMS, RGBA = range(18)


def bare(cls, objective=None, tv=(0.0, 0.0), **rgba):
    """an optimiser without a field behind it: what accumulate() and objective_terms() read, and for train_step() the rows of one
    slot (K = 1) on the host"""
    opt = object.__new__(cls)
    opt.field = types.SimpleNamespace(device=torch.device("cpu"), cell_size=(0.1, 0.1, 0.1))
    opt._rgba = RgbaTargets(**rgba)
    opt.step, opt.white_background, opt.termination, opt.lanes_per_ray = STEP, opt._rgba.white, TERMINATION, LANES
    opt.objective, opt._terms = objective, None
    opt._c = _lib.KnerfBakedTrain() if cls is baked_train.BakedFieldOptimizer else _lib.KnerfBakedBricksTrain()
    opt.learning_rate_sigma, opt.learning_rate_sh, opt.beta_1, opt.beta_2, opt.epsilon = 0.05, 0.01, 0.9, 0.999, 1e-7
    opt.tv_sigma, opt.tv_sh, opt.tv_epsilon, opt.last_regularizer = tv[0], tv[1], 1e-6, None
    opt.iterations, opt.n_slots, opt._width = 0, 1, 4
    opt._master = torch.zeros((1, 4))
    opt._grad, opt._m, opt._v = torch.zeros((1, 4)), torch.zeros((1, 4)), torch.zeros((1, 4))
    opt._point_of, opt._trainable = torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.uint8)
    opt._flags, opt._keys = torch.full((1,), 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    return opt


def rays(n=N):
    rng = np.random.default_rng(2)
    return rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32), np.linspace(1.0, 2.0, n, dtype=np.float32)


HUBER = dict(loss=losses.Huber(0.125), regularizers={"distortion": 0.25, "opacity_entropy": 0.0625})
# (route, objective keywords, rgba keywords, target columns, per-call background) -> what the rgba record must hold
ROUTES = [("", {}, {}, 3, False), ("", dict(loss="mse"), {}, 3, False),
          ("_ext", HUBER, {}, 3, False), ("_ext", dict(loss="mae"), {}, 3, False),
          ("_rgba", {}, dict(opacity_loss=0.25), 4, False), ("_rgba", HUBER, dict(target_background="black"), 4, False),
          ("_rgba", {}, {}, 3, True), ("_rgba", HUBER, dict(opacity_loss=0.5, target_background="white"), 4, True)]


@pytest.mark.parametrize("cls,stem,_tv,_apply", CLASSES)
@pytest.mark.parametrize("route,objective_kw,rgba_kw,columns,per_call", ROUTES)
def test_accumulate_reaches_its_entry_point_with_these_arguments(lib, cls, stem, _tv, _apply, route, objective_kw, rgba_kw, columns,
                                                                 per_call):
    o, d, far = rays()
    target = np.full((N, columns), 0.5, np.float32)
    extra = dict(background=np.full((N, 3), 0.25, np.float32)) if per_call else {}
    objective = check_objective(objective_kw.get("loss"), objective_kw.get("regularizers"))
    opt = bare(cls, objective, white_background=True, **rgba_kw)
    loss = opt.accumulate(o, d, NEAR, far, target, n_total=N_TOTAL, **extra)
    assert loss.dtype == torch.float64 and loss.dim() == 0
    assert lib.names == [stem + route]
    name, a = lib.calls[0]
    assert len(a) == len(_lib.SIGNATURES[name][1]) == {"": 15, "_ext": 17, "_rgba": 18}[route]
    assert a[STREAM] is None and a[STATE] is True and a[O] and a[D] and a[TARGET] and a[SQ]
    assert a[NEAR_T] is None and a[NEAR_ALL] == NEAR and a[FAR_T]
    assert a[N_RAYS] == N and a[N_NORM] == N_TOTAL
    assert a[H] == float(np.float32(STEP)) and a[TERM] == float(np.float32(TERMINATION))
    assert a[FLAGS] == _lib.BAKED_WHITE_BACKGROUND | _lib.BAKED_SKIP_EMPTY | LANES << _lib.BAKED_LANES_SHIFT
    if route:
        assert a[TERMS]
        loss_from, reg = losses.loss_from(objective_kw.get("loss")), objective_kw.get("regularizers") or {}
        want = None if route == "_rgba" and not objective_kw else \
            dict(loss_kind=int(loss_from.kind), huber_delta=float(np.float32(0.125 if loss_from.kind == _lib.LOSS_HUBER else 0.0)),
                 distortion=float(np.float32(reg.get("distortion", 0.0))), opacity_entropy=float(np.float32(reg.get("opacity_entropy", 0.0))))
        assert a[OBJECTIVE] == want
        assert tuple(opt.objective_terms()) == TERM_NAMES + (("opacity",) if route == "_rgba" else ())
    else:
        assert opt.objective_terms() is None
    if route == "_rgba":
        rec = a[RGBA]
        assert (rec["background"] is not None) == per_call and (rec["alpha"] is not None) == (columns == 4)
        assert rec["opacity"] == float(np.float32(rgba_kw.get("opacity_loss", 0.0)))
        assert rec["stored_background"] == (0.0 if rgba_kw.get("target_background") == "black" else 1.0)      # default: the white flag
        assert (opt.last_background is not None) == per_call


@pytest.mark.parametrize("cls,stem,_tv,_apply", CLASSES)
@pytest.mark.parametrize("route,objective_kw,rgba_kw,columns,per_call", ROUTES)
def test_no_rays_no_launch(lib, cls, stem, _tv, _apply, route, objective_kw, rgba_kw, columns, per_call):
    o, d, far = rays(0)
    extra = dict(background=np.zeros((0, 3), np.float32)) if per_call else {}
    opt = bare(cls, check_objective(objective_kw.get("loss"), objective_kw.get("regularizers")), white_background=True, **rgba_kw)
    loss = opt.accumulate(o, d, NEAR, far, np.zeros((0, columns), np.float32), **extra)
    assert lib.calls == [] and loss.dtype == torch.float64 and float(loss) == 0.0
    assert (opt.objective_terms() is None) == (route == "")


@pytest.mark.parametrize("cls,stem,tv,apply", CLASSES)
def test_a_train_step_launches_in_this_order(lib, cls, stem, tv, apply):
    o, d, far = rays()
    target = np.full((N, 3), 0.5, np.float32)
    for weights in ((0.0, 0.0), (1e-3, 0.0), (0.0, 1e-3)):
        lib.calls.clear()
        opt = bare(cls, tv=weights)
        loss = opt.train_step(o, d, NEAR, far, target)
        regularized = tv is not None and max(weights) > 0.0
        assert lib.names == ([stem, tv, apply] if regularized else [stem, apply]), (cls.__name__, weights)
        assert loss.dtype == torch.float64 and opt.iterations == 1
        assert (opt.last_regularizer is not None) == regularized
        for name, a in lib.calls:
            assert len(a) == len(_lib.SIGNATURES[name][1]) and a[0] is None and a[1] is True
        if regularized:
            ws, wc, eps = lib.calls[1][1][-4:-1]
            assert (ws, wc, eps) == (float(np.float32(weights[0] / 1.0)), float(np.float32(weights[1] / 3.0)), float(np.float32(1e-6)))
        rs, rc, b1, b2, eps = lib.calls[-1][1][-5:]
        root = float(np.sqrt(1.0 - 0.999))                                     # Keras-form bias correction at t = 1
        assert (rs, rc) == (float(np.float32(0.05 * root / (1.0 - 0.9))), float(np.float32(0.01 * root / (1.0 - 0.9))))
        assert (b1, b2, eps) == (float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-7)))


TV_KEYS = ["tv_sigma", "tv_sh"]
# (objective keywords, tv weights, rgba keywords and 4-column targets) -> keys
FIT_CASES = [({}, (0.0, 0.0), None), ({}, (1e-3, 1e-3), None), (dict(loss="huber"), (0.0, 0.0), None),
             ({}, (0.0, 1e-3), dict(opacity_loss=0.1))]


@pytest.mark.parametrize("cls,stem,tv,_apply", CLASSES)
@pytest.mark.parametrize("objective_kw,weights,rgba_kw", FIT_CASES)
@pytest.mark.parametrize("n_batches", [2, 0])
def test_fit_returns_these_keys(lib, cls, stem, tv, _apply, objective_kw, weights, rgba_kw, n_batches):
    o, d, far = rays()
    target = np.full((N, 3 if rgba_kw is None else 4), 0.5, np.float32)
    opt = bare(cls, check_objective(objective_kw.get("loss"), None), tv=weights, **(rgba_kw or {}))
    out = opt.fit([(target, (o, d, None))] * n_batches, NEAR, far)
    want = ["loss"] + (TV_KEYS if tv is not None and max(weights) > 0.0 else [])
    if objective_kw or (rgba_kw is not None and n_batches):            # a non-plain objective, or rgba launches were made
        want += list(TERM_NAMES) + (["opacity"] if rgba_kw is not None else [])
    assert list(out) == want, (cls.__name__, list(out))
    assert all(isinstance(v, list) and len(v) == n_batches for v in out.values())
    assert len([n for n in lib.names if n.startswith(stem)]) == n_batches and opt.iterations == n_batches
    # steps= cuts the batches short and is checked before the first launch
    lib.calls.clear()
    assert len(opt.fit([(target, (o, d, None))] * 3, NEAR, far, steps=1)["loss"]) == 1
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            opt.fit([], NEAR, far, steps=bad)


# ---- every keyword arrives under its own name
def _sentinels(white):
    """a distinct value per optimiser keyword, each of which passes the checks; white_background=True allows no background colour, so
    there are two sets"""
    return dict(learning_rate_sigma=0.011, learning_rate_sh=0.022, beta_1=0.33, beta_2=0.44, epsilon=5.5e-5, dilation=6, step=0.077,
                white_background=white, termination=0.088, lanes_per_ray=4, tv_sigma=0.099, tv_sh=0.111, tv_epsilon=1.2e-4,
                loss=losses.Huber(0.13), regularizers=losses.RayRegularizers(distortion=0.14, opacity_entropy=0.15),
                background=None if white else (0.16, 0.17, 0.18), opacity_loss=0.19, target_background="black" if white else "white",
                background_seed=21)


def _constructors():
    return [("BakedField.optimizer", BakedField.optimizer, BakedField), ("BakedFieldOptimizer", baked_train.BakedFieldOptimizer, BakedField),
            ("brick_optimizer", baked_train.brick_optimizer, BrickBakedField),
            ("BrickFieldOptimizer", baked_bricks_train.BrickFieldOptimizer, BrickBakedField),
            ("grid_trainer", baked_bricks_grow.grid_trainer, BrickBakedField),
            ("BrickGridTrainer", baked_bricks_grow.BrickGridTrainer, BrickBakedField)]


def _optimizer_in(exc):
    """the optimiser under construction when `exc` was raised: the innermost `self` of the traceback that is one"""
    found, tb = None, exc.__traceback__
    while tb is not None:
        s = tb.tb_frame.f_locals.get("self")
        if isinstance(s, (baked_train.BakedFieldOptimizer, baked_bricks_train.BrickFieldOptimizer)):
            found = s
        tb = tb.tb_next
    return found


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("by_position", [True, False])
def test_every_keyword_arrives_under_its_own_name(monkeypatch, white, by_position):
    """the source is a stand-in that has its SH degree (the lane check reads it) and nothing else: construction ends with an
    AttributeError at the first other attribute, after every keyword has been checked and stored"""
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    sent = _sentinels(white)
    for name, make, source_type in _constructors():
        source = object.__new__(source_type)
        source.sh_degree = 2
        names = list(inspect.signature(make).parameters)[1:]
        assert set(names) == set(sent) - (set() if "tv_sigma" in names else {"tv_sigma", "tv_sh", "tv_epsilon"}), name
        with pytest.raises(AttributeError) as err:
            make(source, *[sent[k] for k in names]) if by_position else make(source, **{k: sent[k] for k in names})
        opt = _optimizer_in(err.value)
        assert opt is not None, name
        got = {k: getattr(opt, k) for k in names if k in ("learning_rate_sigma", "learning_rate_sh", "beta_1", "beta_2", "epsilon", "dilation",
                                                           "step", "termination", "lanes_per_ray", "tv_sigma", "tv_sh", "tv_epsilon")}
        assert got == {k: sent[k] for k in got}, name
        assert opt.white_background is white and opt._rgba.white is white
        assert losses.record_tuple(opt.objective) == (_lib.LOSS_HUBER, float(np.float32(0.13)), float(np.float32(0.14)),
                                                      float(np.float32(0.15)), 3), name
        r = opt._rgba
        assert (r.mode, r.colour, r.opacity, r.stored, r.seed) == \
            ((None, None, 0.19, 0.0, 21) if white else ("colour", (0.16, 0.17, 0.18), 0.19, 1.0, 21)), name
