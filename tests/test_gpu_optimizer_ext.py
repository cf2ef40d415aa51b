"""The optimizer extensions behind knerf_set_optimizer (csrc/optim_ext.hip): learning-rate schedules, gradient clipping, decoupled
weight decay, and the optimizer state (knerf_get_adam_state / knerf_set_adam_state), against float64 references with INJECTED gradients
(knerf_grads_device is caller-writable by design, as in tests/test_gpu_optimizer.py).

Inputs, cases and tolerances come from tests/optimizer_ext_reference.py; tests/test_optimizer_ext_host.py proves on the CPU, for exactly
these cases and shapes, that the tolerance (8 x the error of float32 arithmetic itself on the same inputs) lies more than ten times below
what any of fifteen deliberate mistakes would produce.  Every comparison runs over ALL elements of both nets, at the default shape
(595,844 parameters: the last workgroup is partial, 170 sum-of-squares items per net), at 4 x 64 / 2 (small, unaligned tensors) and at
4 x 48 zero-padded to 64.

Measured figures: none yet -- this file has not run on an MI355X (no device was available when it was written); each comparison
prints its error and tolerance before it asserts (pytest -s)."""
import numpy as np
import pytest
import torch

from tests import adam_reference as A
from tests import optimizer_ext_reference as X
from tests import optimizer_state_check as S
from tests.test_gpu_forward import log_stats

pytestmark = pytest.mark.gpu
LR, B1, B2, EPS = X.HYPER


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def spec_of(case=None, **kw):
    from keras_nerf_amd.optimizers import OptimizerSpec
    if case is None:
        return OptimizerSpec(lr=kw.pop("lr", LR), beta1=B1, beta2=B2, epsilon=EPS, **kw)
    c = X.CASES[case]
    clip = c["clip"] or (None, 0.0)
    return OptimizerSpec(lr=LR, beta1=B1, beta2=B2, epsilon=EPS, schedule=X.schedule_object(c["sched"]), clip=clip[0], clip_arg=clip[1],
                         weight_decay=c["wd"])


def new_ctx(shape, weights=None, lr=LR, **kw):
    from keras_nerf_amd.runtime import KnerfContext
    ctx = KnerfContext(white_background=True, lr=lr, beta1=B1, beta2=B2, epsilon=EPS, **X.SHAPES[shape], **kw)
    n = int(X.tensor_offsets(**X.SHAPES[shape])[-1])
    assert ctx.param_count == n
    assert (ctx._pad_index is not None) == (shape == "4x48"), shape
    if not kw.get("force_generic"):
        assert ctx.get_option("general_shape_path") == 0.0, shape
    for net in (0, 1):
        ctx.set_weights(net, A.start_weights(n, A.W0_SEEDS[net]) if weights is None else weights[net])
    return ctx


def run_case(ctx, case, shape, label):
    """one case of X.CASES through apply_adam: after EVERY step both nets within the tolerance of float64, the always-zero class
    bit-identical to w0 (or, with weight decay, on w0 prod(1 - wd lr_k)), the accumulator zero, the step count right"""
    from keras_nerf_amd.runtime import NonFiniteGradientError
    (nets, t0, skip, off), ref, tol = X.reference_and_tolerance(case, shape)
    wd = X.CASES[case]["wd"]
    K = len(nets[0][1])
    worst = [0.0, 0.0]
    applied = t0
    for k in range(K):
        gc, gf = nets[0][1][k], nets[1][1][k]
        if k in skip:                                   # alternate the poisoned half, as tests/test_gpu_optimizer.py
            if len([s for s in skip if s <= k]) % 2:
                gc = gc.copy(); gc[gc.size // 3] = float("nan")
            else:
                gf = gf.copy(); gf[gf.size // 3] = float("-inf")
            S.inject(ctx, gc, gf)
            with pytest.raises(NonFiniteGradientError):
                ctx.apply_adam()
        else:
            S.inject(ctx, gc, gf)
            ctx.apply_adam()
            applied += 1
        assert ctx.step == applied, (label, k)
        assert not bool(ctx.grads_view().view(torch.int32).any()), (label, k, "accumulator not zero")
        for net in (0, 1):
            w = ctx.get_weights(net)
            err = float(np.abs(w - ref[k][net]).max())
            worst[net] = max(worst[net], err)
            print(f"{label} step {k} net {net}: |w - fp64| = {err:.3e}, tolerance {tol[net]:.3e}")
            assert err <= tol[net], (label, "step", k, "net", net, err, tol[net])
            w0, _, cls = nets[net]
            z = cls == A.ZERO
            if wd > 0:
                pure = X.pure_decay(case, w0[z], t0, skip, K)[k]
                assert np.abs(w[z] - pure).max() <= tol[net], (label, k, net, "always-zero class off pure decay")
            else:
                assert np.array_equal(u32(w[z]), u32(w0[z])), (label, k, net, "always-zero class moved")
    log_stats(f"optimizer_ext_{label}", worst_coarse=worst[0], worst_fine=worst[1], tol_coarse=tol[0], tol_fine=tol[1])
    return worst, tol


def drive(ctx, shape, base="trajectory", steps=None, scale_fine=None):
    """inject the gradient schedule of a base case step by step; returns the weights of both nets after every step"""
    n = ctx.param_count
    G = [A.case_inputs(base, net, n)[1] for net in (0, 1)]
    out = []
    for k in range(len(G[0]) if steps is None else steps):
        S.inject(ctx, G[0][k], G[1][k] if scale_fine is None else scale_fine(G[0][k]))
        ctx.apply_adam()
        out.append([ctx.get_weights(net) for net in (0, 1)])
    return out


# ---- 1.-3. schedules, clipping, weight decay against float64 -------------------------------------------------------------------------

@pytest.mark.parametrize("shape,case", X.GPU_RUNS, ids=[f"{s}-{c}" for s, c in X.GPU_RUNS])
def test_extended_update_follows_fp64(shape, case):
    """Schedules (exponential continuous and staircase, cosine with four steps behind the clamp, piecewise; the skipped-step and resume
    cases under the exponential schedule), each clip kind with a threshold that always clips, the large-gradient case (1,000 entries of
    +-1e18 in one tensor: a finite factor needs the double sum), weight decay alone and with schedule and global clipping together."""
    ctx = new_ctx(shape)
    try:
        t0 = A.CASES[X.CASES[case]["base"]][1]
        if shape == "4x64":                 # the two orders: knerf_set_optimizer re-derives the rate from the device-side count,
            if t0:
                ctx.step = t0
            ctx.set_optimizer(spec_of(case))
        else:                               # knerf_set_step_count re-derives it from the schedule
            ctx.set_optimizer(spec_of(case))
            if t0:
                ctx.step = t0
        run_case(ctx, case, shape, f"{shape}_{case}")
    finally:
        ctx.close()


@pytest.mark.parametrize("case", X.GENERIC_CASES)
def test_general_shape_path_takes_the_same_kernels(case):
    ctx = new_ctx("default", force_generic=True)
    try:
        assert ctx.get_option("general_shape_path") == 1.0
        ctx.set_optimizer(spec_of(case))
        run_case(ctx, case, "default", f"generic_{case}")
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", list(X.SHAPES))
def test_a_rate_of_zero_leaves_the_weights_in_their_bits(shape):
    """piecewise, boundaries 3 and 7, last value 0.0: the steps of index >= 8 change no bit of either net (their moments still move)"""
    ctx = new_ctx(shape)
    try:
        ctx.set_optimizer(spec_of(schedule=X.schedule_object(X.SCHEDULES["piecewise_zero"])))
        W = drive(ctx, shape)
        m_before = ctx.get_adam_state(0)[0]
        for net in (0, 1):
            assert not np.array_equal(u32(W[7][net]), u32(W[6][net])), (shape, net, "step 7 (rate 5e-4) did not move")
            for k in range(8, len(W)):
                assert np.array_equal(u32(W[k][net]), u32(W[7][net])), (shape, net, k)
        n = ctx.param_count
        S.inject(ctx, A.gradient_schedule(n, 1, 77)[0][0], A.gradient_schedule(n, 1, 78)[0][0])
        ctx.apply_adam()
        assert np.array_equal(u32(ctx.get_weights(0)), u32(W[7][0]))
        assert not np.array_equal(u32(ctx.get_adam_state(0)[0]), u32(m_before))
    finally:
        ctx.close()


_PLAIN = {}


def plain_trajectory(shape):
    """the plain path's weights after every step of the trajectory case on an untouched context (once per shape)"""
    if shape not in _PLAIN:
        ctx = new_ctx(shape)
        try:
            _PLAIN[shape] = drive(ctx, shape)
            assert ctx.get_optimizer().schedule == 0 and ctx.get_optimizer().lr == float(np.float32(LR))
        finally:
            ctx.close()
    return _PLAIN[shape]


@pytest.mark.parametrize("kind", list(X.CLIP_NEVER))
@pytest.mark.parametrize("shape", list(X.SHAPES))
def test_a_threshold_that_never_clips_is_the_plain_path_bit_for_bit(shape, kind):
    """the factor is exactly 1.0f where nothing is clipped: the extended kernels then give the plain kernels' bits at every step"""
    plain = plain_trajectory(shape)
    ctx = new_ctx(shape)
    try:
        ctx.set_optimizer(spec_of(clip=kind, clip_arg=X.CLIP_NEVER[kind]))
        got = drive(ctx, shape)
        for k, (a, b) in enumerate(zip(got, plain)):
            for net in (0, 1):
                assert np.array_equal(u32(a[net]), u32(b[net])), (shape, kind, "step", k, "net", net)
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", list(X.SHAPES))
def test_clipped_runs_repeat_bit_for_bit(shape):
    """no floating-point atomics in the norms: per-workgroup partial sums, then an ordered pass"""
    for kind in ("clipnorm", "global_clipnorm"):
        runs = []
        for _ in range(2):
            ctx = new_ctx(shape)
            try:
                ctx.set_optimizer(spec_of(clip=kind, clip_arg=X.CLIP_ALWAYS[kind]))
                runs.append(drive(ctx, shape, steps=4)[-1])
            finally:
                ctx.close()
        for net in (0, 1):
            assert np.array_equal(u32(runs[0][net]), u32(runs[1][net])), (shape, kind, net)


@pytest.mark.parametrize("shape", list(X.SHAPES))
def test_global_clipnorm_takes_each_nets_own_norm(shape):
    """Both nets start from the same weights; the fine net gets the coarse gradient times 4.  Its norm is then exactly 4 times the
    coarse one, its factor exactly a quarter, its clipped gradient the coarse one's bits -- if and only if each net is scaled by its
    OWN norm.  (A norm over both nets would give both the same factor and the fine net a gradient four times as large.)"""
    n = int(X.tensor_offsets(**X.SHAPES[shape])[-1])
    w0 = A.start_weights(n, A.W0_SEEDS[0])
    ctx = new_ctx(shape, weights=[w0, w0])
    try:
        ctx.set_optimizer(spec_of(clip="global_clipnorm", clip_arg=X.CLIP_ALWAYS["global_clipnorm"]))
        W = drive(ctx, shape, steps=4, scale_fine=lambda g: g * np.float32(4))
        for k, (c, f) in enumerate(W):
            assert np.array_equal(u32(c), u32(f)), (shape, k)
        assert not np.array_equal(u32(W[-1][0]), u32(w0))
    finally:
        ctx.close()
    # ... and without clipping the two nets do differ on these inputs (the test can tell)
    ctx = new_ctx(shape, weights=[w0, w0])
    try:
        ctx.set_optimizer(spec_of(clip="global_clipnorm", clip_arg=X.CLIP_NEVER["global_clipnorm"]))
        c, f = drive(ctx, shape, steps=4, scale_fine=lambda g: g * np.float32(4))[-1]
        assert not np.array_equal(u32(c), u32(f))
    finally:
        ctx.close()


# ---- 4. state and no-regression ------------------------------------------------------------------------------------------------------

def test_a_constant_schedule_and_nothing_else_selects_the_plain_kernels():
    """knerf_set_optimizer(constant, no clip, no decay) = an untouched context over the trajectory case, bit for bit"""
    plain = plain_trajectory("default")
    ctx = new_ctx("default")
    try:
        ctx.set_optimizer(spec_of())
        o = ctx.get_optimizer()
        assert (o.schedule, o.clip, o.weight_decay, o.lr) == (0, 0, 0.0, float(np.float32(LR)))
        got = drive(ctx, "default")
        for k, (a, b) in enumerate(zip(got, plain)):
            for net in (0, 1):
                assert np.array_equal(u32(a[net]), u32(b[net])), ("step", k, "net", net)
    finally:
        ctx.close()


def test_invalid_optimizer_records_are_refused():
    from keras_nerf_amd import _lib
    ctx = new_ctx("4x64")
    try:
        def rec(**kw):
            o = spec_of().to_struct()
            for k, v in kw.items():
                if isinstance(v, (list, tuple)):
                    for i, x in enumerate(v):
                        getattr(o, k)[i] = x
                else:
                    setattr(o, k, v)
            return o
        bad = [rec(clip=_lib.CLIP_VALUE | _lib.CLIP_NORM, clip_arg=1.0), rec(clip=8, clip_arg=1.0), rec(clip=_lib.CLIP_NORM, clip_arg=0.0),
               rec(schedule=_lib.SCHEDULE_EXPONENTIAL, decay_steps=0.0, decay_rate=0.5), rec(schedule=_lib.SCHEDULE_COSINE, decay_steps=-1.0),
               rec(schedule=_lib.SCHEDULE_PIECEWISE, n_values=3, boundaries=[5, 5], values=[1e-3, 1e-4, 1e-5]),
               rec(schedule=_lib.SCHEDULE_PIECEWISE, n_values=17), rec(schedule=_lib.SCHEDULE_PIECEWISE, n_values=0),
               rec(schedule=_lib.SCHEDULE_PIECEWISE, n_values=2, boundaries=[5], values=[1e-3, -1e-4]),
               rec(lr=-1e-3), rec(lr=float("nan")), rec(weight_decay=float("inf")), rec(weight_decay=-1.0), rec(schedule=9)]
        for o in bad:
            with pytest.raises(ValueError):
                ctx.set_optimizer(o)
            assert ctx.lib.knerf_last_error(ctx._ctx)
        assert ctx.get_optimizer().schedule == 0 and ctx.get_optimizer().clip == 0          # nothing of them was kept
    finally:
        ctx.close()


def test_set_learning_rate_and_state_resume():
    """K steps, then the whole state (weights, m, v, step count) into a fresh context, then K more: the bits of 2 K uninterrupted
    steps.  And a new constant rate set between steps acts like a context created with that rate and given the same state."""
    shape, K = "default", 3
    n = int(X.tensor_offsets(**X.SHAPES[shape])[-1])
    G = [A.case_inputs("trajectory", net, n)[1] for net in (0, 1)]

    def steps(ctx, ks):
        for k in ks:
            S.inject(ctx, G[0][k], G[1][k])
            ctx.apply_adam()

    def carry(src, dst):
        for net in (0, 1):
            dst.set_weights(net, src.get_weights(net))
            dst.set_adam_state(net, *src.get_adam_state(net))
        dst.step = src.step

    a, b, c = new_ctx(shape), None, None
    try:
        steps(a, range(K))
        m, v = a.get_adam_state(0)
        assert m.size == n and np.abs(m).max() > 0 and v.min() >= 0 and v.max() > 0
        b = new_ctx(shape)
        carry(a, b)
        assert b.step == K
        steps(a, range(K, 2 * K)); steps(b, range(K, 2 * K))
        for net in (0, 1):
            assert np.array_equal(u32(a.get_weights(net)), u32(b.get_weights(net))), net
            for x, y in zip(a.get_adam_state(net), b.get_adam_state(net)):
                assert np.array_equal(u32(x), u32(y))
        plain = plain_trajectory(shape)
        assert np.array_equal(u32(a.get_weights(1)), u32(plain[2 * K - 1][1]))
        # without the slots it is another run
        c = new_ctx(shape, weights=[b.get_weights(0), b.get_weights(1)])
        c.step = 2 * K
        steps(a, [2 * K]); steps(c, [2 * K])
        assert not np.array_equal(u32(a.get_weights(0)), u32(c.get_weights(0)))
        c.close()
        # set_learning_rate: a, after 2 K + 1 steps at 1e-3, continues at 5e-4 == a context CREATED with 5e-4 that is given a's state
        c = new_ctx(shape, lr=5e-4)
        carry(a, c)
        a.set_optimizer(spec_of(lr=5e-4))
        assert a.get_optimizer().lr == float(np.float32(5e-4))
        steps(a, [2 * K + 1]); steps(c, [2 * K + 1])
        for net in (0, 1):
            assert np.array_equal(u32(a.get_weights(net)), u32(c.get_weights(net))), net
        with pytest.raises(ValueError):
            a.set_adam_state(0, m[:-1], v[:-1])
    finally:
        for x in (a, b, c):
            if x is not None:
                x.close()


def _tiny_model(model_path=None, optimizer="adam"):
    from keras_nerf_amd.model.nerf.nerf import NeRF
    nerf = NeRF(model_path=model_path)
    nerf.compile(optimizer, "mse", batch_size=1, image_height=4, image_width=4, ray_chunks=16, white_background=True, deterministic=True)
    return nerf


def test_nerf_saves_and_resumes_the_optimizer_state(tmp_path):
    """save_model(optimizer_state=True) -> NeRF(model_path) -> compile -> load_optimizer_state: the next train_step on the same inputs
    gives the original model's bits; without load_optimizer_state it does not.  The default save writes the reference's files only."""
    import os
    from oracle import nerf_oracle as O
    from tests.problem import make_problem
    from keras_nerf_amd import optimizers as K
    P = make_problem(n_images=1, wh=4)
    batch = (P["img"], (P["o"], P["d"], P["t"]))
    opt = K.Adam(learning_rate=K.schedules.ExponentialDecay(1e-3, 2, 0.5), global_clipnorm=0.5, weight_decay=1e-2)
    nerf = _tiny_model(optimizer=opt)
    nerf.coarse.set_flat_weights(O.flatten_params(P["cp"])); nerf.fine.set_flat_weights(O.flatten_params(P["fp"]))
    assert nerf.learning_rate == 1e-3
    for _ in range(3):
        nerf.train_step(batch, u=P["u"], with_metrics=False)
    assert nerf._ctx.step == 3 and nerf.learning_rate == pytest.approx(1e-3 * 0.5 ** 1.5, rel=1e-15)
    with pytest.raises(ValueError, match="schedule"):
        nerf.set_learning_rate(1e-4)
    plain_dir, full_dir = str(tmp_path / "plain"), str(tmp_path / "full")
    nerf.save_model(plain_dir)
    assert sorted(os.listdir(plain_dir)) == ["coarse.h5", "fine.h5", "model_config.json"]
    nerf.save_model(full_dir, optimizer_state=True)
    assert sorted(os.listdir(full_dir)) == ["coarse.h5", "fine.h5", "model_config.json", "optimizer_state.npz"]
    nerf.train_step(batch, u=P["u"], with_metrics=False)
    want = [nerf.coarse.get_flat_weights(), nerf.fine.get_flat_weights()]
    resumed = _tiny_model(full_dir, opt)
    cfg = resumed.load_optimizer_state(full_dir)
    assert cfg == nerf._opt_spec.get_config() and resumed._ctx.step == 3 and resumed.learning_rate == pytest.approx(1e-3 * 0.5 ** 1.5, rel=1e-15)
    resumed.train_step(batch, u=P["u"], with_metrics=False)
    cold = _tiny_model(full_dir, opt)
    cold.train_step(batch, u=P["u"], with_metrics=False)
    for i, (w, r, c) in enumerate(zip(want, (resumed.coarse, resumed.fine), (cold.coarse, cold.fine))):
        assert np.array_equal(u32(r.get_flat_weights()), u32(w)), ("resumed", i)
        assert not np.array_equal(u32(c.get_flat_weights()), u32(w)), ("cold start", i)
    other = _tiny_model()                                            # the same shape resumes; a different one is refused
    other.load_optimizer_state(full_dir)
    from keras_nerf_amd.model.nerf.nerf import NeRF
    small = NeRF(n_layers=4, dense_units=64, skip_layer=2)
    small.compile("adam", "mse", batch_size=1, image_height=4, image_width=4, ray_chunks=16)
    with pytest.raises(ValueError, match="parameters"):
        small.load_optimizer_state(full_dir)


def test_nerf_trains_under_a_piecewise_schedule_that_ends_at_zero():
    """compile(optimizer=Adam(learning_rate=PiecewiseConstantDecay([2], [1e-3, 0.0]))): steps 0, 1, 2 use 1e-3 (step <= 2), the fourth
    uses 0.0 and leaves every bit; set_learning_rate on a constant-rate model reaches the next step"""
    from oracle import nerf_oracle as O
    from tests.problem import make_problem
    from keras_nerf_amd import optimizers as K
    P = make_problem(n_images=1, wh=4)
    batch = (P["img"], (P["o"], P["d"], P["t"]))
    nerf = _tiny_model(optimizer=K.Adam(learning_rate=K.schedules.PiecewiseConstantDecay([2], [1e-3, 0.0])))
    nerf.coarse.set_flat_weights(O.flatten_params(P["cp"])); nerf.fine.set_flat_weights(O.flatten_params(P["fp"]))
    W = [[nerf.coarse.get_flat_weights(), nerf.fine.get_flat_weights()]]
    rates = []
    for _ in range(4):
        rates.append(nerf.learning_rate)
        nerf.train_step(batch, u=P["u"], with_metrics=False)
        W.append([nerf.coarse.get_flat_weights(), nerf.fine.get_flat_weights()])
    assert rates == [1e-3, 1e-3, 1e-3, 0.0]
    for net in (0, 1):
        for k in range(3):
            assert not np.array_equal(u32(W[k + 1][net]), u32(W[k][net])), (net, k)
        assert np.array_equal(u32(W[4][net]), u32(W[3][net])), net
    const = _tiny_model(optimizer=K.Adam(1e-3))
    const.coarse.set_flat_weights(O.flatten_params(P["cp"])); const.fine.set_flat_weights(O.flatten_params(P["fp"]))
    const.set_learning_rate(0.0)
    assert const.learning_rate == 0.0
    const.train_step(batch, u=P["u"], with_metrics=False)
    assert np.array_equal(u32(const.coarse.get_flat_weights()), u32(O.flatten_params(P["cp"])))
    const.set_learning_rate(1e-3)
    const.train_step(batch, u=P["u"], with_metrics=False)
    assert not np.array_equal(u32(const.coarse.get_flat_weights()), u32(O.flatten_params(P["cp"])))
