"""What tests/test_gpu_optimizer_ext.py rests on, proved on the CPU (no GPU needed) for exactly the cases of
tests/optimizer_ext_reference.py: every deliberate mistake differs from the float64 reference by more than POWER_FACTOR x the
tolerance (TOL_FACTOR x the fp32 mirrors' own error) on at least one case where it can differ at all; the schedule classes, the
optimizer parser, the configuration round trip and the optimizer_state.npz round trip."""
import json
import math

import numpy as np
import pytest

from tests import adam_reference as A
from tests import optimizer_ext_reference as X

# every case of X.CASES at every shape the GPU file runs
SHAPES_RUN = tuple(X.SHAPES)


@pytest.fixture(scope="module")
def measured():
    """{(shape, case): (tolerances, {mutant: worst distance per net})}, computed once"""
    out = {}
    for shape in SHAPES_RUN:
        for case in X.CASES:
            inp, ref, tol = X.reference_and_tolerance(case, shape)
            out[(shape, case)] = (tol, {m: X.worst(X.update(case, *inp, mutant=m), ref) for m in X.mutants_for(case)})
    return out


def test_every_case_has_a_usable_tolerance(measured):
    """the mirrors' error is what fp32 costs on these inputs: positive, and small against the movement of the weights"""
    for (shape, case), (tol, _) in measured.items():
        for t in tol:
            assert 0 < t < 5e-5, (shape, case, tol)


@pytest.mark.parametrize("mutant", X.MUTANTS)
def test_each_mistake_is_far_outside_the_tolerance(measured, mutant):
    seen, separated = 0, []
    for (shape, case), (tol, dist) in measured.items():
        if mutant not in dist:
            continue
        seen += 1
        ratio = max(d / t for d, t in zip(dist[mutant], tol))
        print(f"{mutant} on {shape}/{case}: {ratio:.1f} x tolerance")
        if ratio > X.POWER_FACTOR:
            separated.append((shape, case))
    assert seen, f"no case can show {mutant}"
    assert separated, f"{mutant} stays within {X.POWER_FACTOR} x the tolerance on every case"
    # and at every shape, so that no shape's run is blind to it
    assert {s for s, _ in separated} == set(SHAPES_RUN), (mutant, separated)


def test_the_mutant_lists_cover_the_issue():
    assert len(X.MUTANTS) == 15 and len(set(X.MUTANTS)) == 15
    covered = set()
    for case in X.CASES:
        covered |= set(X.mutants_for(case))
    assert covered == set(X.MUTANTS)
    assert X.mutants_for("exp") == ("schedule_at_t",)
    assert "sumsq_fp32" in X.mutants_for("global_clipnorm_large") and "sumsq_fp32" not in X.mutants_for("global_clipnorm")


def test_an_fp32_sum_of_squares_overflows_on_the_large_gradient_case():
    nets, t0, skip, off = X.case_inputs("clipnorm_large", "4x64")
    g = [G[0] for _, G, _ in nets]
    assert all(np.count_nonzero(np.abs(x) == np.float32(X.LARGE_VALUE)) == X.LARGE_COUNT for x in g)
    assert all(np.abs(x).max() <= A.G_CAP for x in g)
    assert not np.isfinite(X._sumsq(g, off, np.float32)[0]).all()
    assert np.isfinite(X._sumsq(g, off, np.float64)[0]).all()
    f = X._clip_factors(g, off, ("clipnorm", 1e-2))[0]
    assert np.isfinite(f).all() and (f > 0).all()


def test_the_always_zero_class_follows_pure_decay():
    for case in X.DECAY_CASES:
        inp, ref, tol = X.reference_and_tolerance(case, "4x64")
        nets, t0, skip, off = inp
        for net, (w0, G, cls) in enumerate(nets):
            z = cls == A.ZERO
            pure = X.pure_decay(case, w0[z], t0, skip, len(G))
            for k in range(len(G)):
                assert np.abs(ref[k][net][z] - pure[k]).max() <= 1e-15


# ---- the schedule classes ----------------------------------------------------------------------------------------------------------

def _steps_around(boundaries):
    s = {0, 10 ** 6}
    for b in boundaries:
        s |= {max(b - 1, 0), b, b + 1}
    return sorted(s)


@pytest.mark.parametrize("name", list(X.SCHEDULES))
def test_schedule_classes_follow_the_formulas(name):
    s = X.SCHEDULES[name]
    obj = X.schedule_object(s)
    bounds = s["boundaries"] if s["kind"] == "piecewise" else (int(s["decay_steps"]), 2 * int(s["decay_steps"]))
    for step in _steps_around(bounds):
        want = X.schedule_lr(s, step)
        got = obj(step)
        assert isinstance(got, float)
        assert got == pytest.approx(want, rel=1e-15, abs=0), (name, step)
    # spot values written out by hand
    if name == "exp":
        assert obj(4) == pytest.approx(5e-4, rel=1e-15) and obj(2) == pytest.approx(1e-3 * math.sqrt(0.5), rel=1e-15)
    if name == "exp_stair":
        assert obj(3) == 1e-3 and obj(4) == 5e-4 and obj(7) == 5e-4 and obj(8) == 2.5e-4
    if name == "cosine":
        assert obj(0) == pytest.approx(1e-3, rel=1e-15) and obj(8) == pytest.approx(1e-4, rel=1e-12) and obj(9) == obj(8) == obj(10 ** 6)
        assert obj(4) == pytest.approx(1e-3 * (0.9 * 0.5 + 0.1), rel=1e-12)
    if name == "piecewise":
        assert [obj(k) for k in (0, 3, 4, 7, 8, 100)] == [1e-3, 1e-3, 5e-4, 5e-4, 1e-4, 1e-4]


def test_schedule_classes_refuse_bad_arguments():
    from keras_nerf_amd import optimizers as K
    for make in (lambda: K.ExponentialDecay(1e-3, 0, 0.5), lambda: K.ExponentialDecay(-1e-3, 4, 0.5), lambda: K.CosineDecay(1e-3, -2),
                 lambda: K.CosineDecay(1e-3, 8, warmup_steps=5), lambda: K.PiecewiseConstantDecay([3, 3], [1, 2, 3]),
                 lambda: K.PiecewiseConstantDecay([3], [1.0]), lambda: K.PiecewiseConstantDecay(list(range(16)), [1.0] * 17),
                 lambda: K.PiecewiseConstantDecay([2], [1.0, float("nan")]), lambda: K.ExponentialDecay(float("inf"), 4, 0.5)):
        with pytest.raises(ValueError):
            make()


# ---- the parser --------------------------------------------------------------------------------------------------------------------

def test_parser_accepts_what_this_build_implements():
    from keras_nerf_amd import optimizers as K
    from keras_nerf_amd.model.nerf.nerf import _adam_hyper, _optimizer_spec
    for plain in (None, "adam", "Adam", {"learning_rate": 2e-4, "beta_1": 0.8, "beta_2": 0.99, "epsilon": 1e-8}, K.Adam(), K.Adam(5e-4)):
        sp = _optimizer_spec(plain)
        assert sp.is_plain
        h = _adam_hyper(plain)                       # the plain case IS _adam_hyper's
        assert (sp.lr, sp.beta1, sp.beta2, sp.epsilon) == (h["lr"], h["beta1"], h["beta2"], h["epsilon"])
    sp = _optimizer_spec(K.Adam(learning_rate=K.schedules.ExponentialDecay(5e-4, 1000, 0.1, staircase=True), beta_1=0.8))
    assert not sp.is_plain and isinstance(sp.schedule, K.ExponentialDecay) and sp.beta1 == 0.8 and sp.lr == 5e-4
    assert sp.lr_at(999) == 5e-4 and sp.lr_at(1000) == pytest.approx(5e-5)
    for kind in ("clipnorm", "clipvalue", "global_clipnorm"):
        sp = _optimizer_spec(K.Adam(**{kind: 0.5}))
        assert (sp.clip, sp.clip_arg, sp.is_plain) == (kind, 0.5, False)
    sp = _optimizer_spec(K.Adam(weight_decay=4e-3))
    assert sp.weight_decay == 4e-3 and not sp.is_plain
    assert _optimizer_spec(K.Adam(weight_decay=0.0, clipnorm=None)).is_plain

    class CosineDecay:                               # a foreign object with the Keras class name and get_config(): a tf.keras schedule
        def get_config(self):
            return {"initial_learning_rate": 1e-3, "decay_steps": 8, "alpha": 0.1, "name": "CosineDecay", "warmup_target": None, "warmup_steps": 0}

    class Adam:                                      # duck-typed tf.keras.optimizers.Adam, Keras 3 get_config keys
        def get_config(self):
            return {"name": "adam", "learning_rate": {"module": "keras.optimizers.schedules", "class_name": "CosineDecay",
                                                      "config": CosineDecay().get_config(), "registered_name": None},
                    "weight_decay": 1e-2, "clipnorm": None, "global_clipnorm": 1.0, "clipvalue": None, "use_ema": False, "ema_momentum": 0.99,
                    "ema_overwrite_frequency": None, "loss_scale_factor": None, "gradient_accumulation_steps": None,
                    "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "amsgrad": False}
    sp = _optimizer_spec(Adam())
    assert isinstance(sp.schedule, K.CosineDecay) and sp.clip == "global_clipnorm" and sp.weight_decay == 1e-2
    assert sp.lr_at(4) == pytest.approx(X.schedule_lr(X.SCHEDULES["cosine"], 4), rel=1e-15)

    class WithAttributes:                            # attributes only, no get_config
        learning_rate = CosineDecay()
        clipvalue = 2.0
    WithAttributes.__name__ = "Adam"
    sp = _optimizer_spec(WithAttributes())
    assert isinstance(sp.schedule, K.CosineDecay) and (sp.clip, sp.clip_arg) == ("clipvalue", 2.0)


def test_parser_refuses_the_rest_naming_the_option():
    from keras_nerf_amd import optimizers as K
    from keras_nerf_amd.model.nerf.nerf import _optimizer_spec
    bad = [
        (K.Adam(amsgrad=True), "amsgrad"), (K.Adam(use_ema=True), "use_ema"),
        (K.Adam(clipnorm=1.0, clipvalue=1.0), "clipnorm"), (K.Adam(global_clipnorm=1.0, clipvalue=1.0), "global_clipnorm"),
        (K.Adam(learning_rate=lambda step: 1e-3), "learning_rate"),
        (K.Adam(learning_rate={"class_name": "InverseTimeDecay", "config": {}}), "InverseTimeDecay"),
        (K.Adam(learning_rate={"class_name": "CosineDecay", "config": {"initial_learning_rate": 1e-3, "decay_steps": 8, "warmup_steps": 3}}), "warm"),
        (K.Adam(clipnorm=-1.0), "clipnorm"), (K.Adam(clipvalue=0.0), "clipvalue"), (K.Adam(weight_decay=-1e-3), "weight_decay"),
        (K.Adam(weight_decay=float("nan")), "weight_decay"),
        ({"class_name": "SGD", "config": {"learning_rate": 1e-2}}, "SGD"), ("rmsprop", "rmsprop"),
        ({"class_name": "Adam", "config": {"gradient_accumulation_steps": 4}}, "gradient_accumulation_steps"),
        (K.Adam(learning_rate={"class_name": "ExponentialDecay", "config": {"initial_learning_rate": 1e-3, "decay_steps": 0, "decay_rate": 0.5}}), "decay_steps"),
    ]
    for opt, word in bad:
        with pytest.raises(ValueError, match=word):
            _optimizer_spec(opt)


def test_configuration_round_trips_through_get_config_and_the_dict_form():
    from keras_nerf_amd import optimizers as K
    from keras_nerf_amd.model.nerf.nerf import _optimizer_spec
    for sname, s in X.SCHEDULES.items():
        opt = K.Adam(learning_rate=X.schedule_object(s), beta_1=0.85, global_clipnorm=0.25, weight_decay=1e-3)
        cfg = opt.get_config()
        cfg2 = json.loads(json.dumps(cfg))                       # JSON-able
        again = K.Adam.from_config(cfg2)
        assert again.get_config() == cfg
        a, b, c = _optimizer_spec(opt), _optimizer_spec({"class_name": "Adam", "config": cfg2}), _optimizer_spec(again)
        assert a.get_config() == b.get_config() == c.get_config()
        d = _optimizer_spec(json.loads(json.dumps(a.get_config())))        # the spec's own serialised form comes back too
        assert d.get_config() == a.get_config()
        for step in (0, 3, 4, 8, 1000):
            assert a.lr_at(step) == d.lr_at(step) == X.schedule_lr(s, step) or a.lr_at(step) == pytest.approx(X.schedule_lr(s, step), rel=1e-15)
        sched = K.schedule_from(K.serialize_schedule(a.schedule))
        assert type(sched) is type(a.schedule) and sched.get_config() == a.schedule.get_config()


def test_the_abi_record_of_a_spec():
    from keras_nerf_amd import _lib
    from keras_nerf_amd import optimizers as K
    o = K.OptimizerSpec(schedule=X.schedule_object(X.SCHEDULES["piecewise"]), clip="clipnorm", clip_arg=2.0, weight_decay=0.5).to_struct()
    assert (o.schedule, o.n_values, o.clip, o.clip_arg, o.weight_decay) == (_lib.SCHEDULE_PIECEWISE, 3, _lib.CLIP_NORM, 2.0, 0.5)
    assert list(o.boundaries[:2]) == [3, 7] and list(o.values[:3]) == [1e-3, 5e-4, 1e-4]
    o = K.OptimizerSpec(schedule=X.schedule_object(X.SCHEDULES["exp_stair"])).to_struct()
    assert (o.schedule, o.lr, o.decay_steps, o.decay_rate, o.staircase, o.clip) == (_lib.SCHEDULE_EXPONENTIAL, 1e-3, 4.0, 0.5, 1, _lib.CLIP_NONE)
    o = K.OptimizerSpec(lr=2e-4).to_struct()
    assert (o.schedule, o.lr, o.clip, o.weight_decay) == (_lib.SCHEDULE_CONSTANT, 2e-4, 0, 0.0)
    import ctypes as C
    assert C.sizeof(_lib.KnerfOptimizer) == 16 + 6 * 8 + 15 * 8 + 16 * 8           # struct knerf_optimizer, include/knerf.h


# ---- optimizer_state.npz -----------------------------------------------------------------------------------------------------------

def test_optimizer_state_file_round_trips(tmp_path):
    from keras_nerf_amd import optimizers as K
    rng = np.random.default_rng(3)
    n = 1234
    slots = {k: rng.standard_normal(n).astype(np.float32) for k in ("coarse_m", "coarse_v", "fine_m", "fine_v")}
    slots["coarse_v"][:3] = [0.0, np.float32(1e-38), np.float32(3e38)]
    cfg = K.OptimizerSpec(schedule=X.schedule_object(X.SCHEDULES["cosine"]), clip="clipvalue", clip_arg=0.1, weight_decay=1e-2).get_config()
    file = K.save_optimizer_state(str(tmp_path), 4711, slots, cfg)
    assert file.endswith("optimizer_state.npz")
    for where in (str(tmp_path), file):
        step, back, cfg2 = K.load_optimizer_state(where)
        assert step == 4711 and cfg2 == cfg
        for k, v in slots.items():
            assert back[k].dtype == np.float32 and np.array_equal(back[k].view(np.uint32), v.view(np.uint32)), k
    with pytest.raises(ValueError):
        K.save_optimizer_state(str(tmp_path / "x"), 1, dict(slots, fine_v=slots["fine_v"][:-1]), cfg)
    np.savez(str(tmp_path / "other.npz"), step=np.int64(1))
    with pytest.raises(ValueError, match="not an optimizer state"):
        K.load_optimizer_state(str(tmp_path / "other.npz"))
