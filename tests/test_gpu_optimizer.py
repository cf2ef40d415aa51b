"""knerf_apply_adam and everything it re-derives, against float64 references, with INJECTED gradients.

The gradient accumulator is caller-writable by design (knerf_grads_device: what a data-parallel all-reduce writes into), so the
stretch finite check -> Adam (x 2 nets) -> head composition -> bf16 re-packing -> step count can be driven through the product ABI with
gradients the test chooses -- no bf16 noise, nothing of the code under test fed back into the reference.  Inputs, cases and tolerances
come from tests/adam_reference.py; tests/test_adam_host.py proves on the CPU that tol_adam (8 x the error of float32 arithmetic
itself on the same schedule, about 1e-6) is more than ten times below what ANY of ten wrong Adams (epsilon inside the root, torch-form
bias correction, t off by one, a skipped step that advances t, ...) would produce on these very inputs.

Every comparison runs over ALL 595,844 elements of both nets (not a multiple of 256: the last Adam workgroup is partial).  The
tests/test_gpu_train.py Adam test (real gradients, loose) stays: it is the one with gradients from the training kernels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import adam_reference as A
from tests import optimizer_state_check as S
from tests.test_gpu_forward import log_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = O.param_count(O.NerfConfig())


def new_ctx(hyper="default", weights=None, **kw):
    from keras_nerf_amd.runtime import KnerfContext
    lr, b1, b2, eps = A.HYPER[hyper]
    ctx = KnerfContext(white_background=True, lr=lr, beta1=b1, beta2=b2, epsilon=eps, **kw)
    assert ctx.param_count == N and ctx.grads_view().numel() == 2 * N
    for net in (0, 1):
        ctx.set_weights(net, A.start_weights(N, A.W0_SEEDS[net]) if weights is None else weights[net])
    return ctx


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def poisoned(g, where=None, value=float("nan")):
    g = g.copy()
    g[g.size // 3 if where is None else where] = value
    return g


def accumulator_is_zero(ctx):
    return not bool(ctx.grads_view().view(torch.int32).any())          # +0 exactly, every element of both halves


def run_case(ctx, case, hyper, check_every_step=True):
    """drive one case of adam_reference.CASES through apply_adam(check=True); returns per net the worst |w_gpu - fp64| and tol_adam"""
    from keras_nerf_amd.runtime import NonFiniteGradientError
    h = A.HYPER[hyper]
    inp = [A.case_inputs(case, net, N) for net in (0, 1)]
    K, t0, skip = A.CASES[case]
    refs = [A.adam_fp64(w0, G, *h, t0=t0, skip=skip, every_step=True) for w0, G, _, _, _ in inp]
    tols = [A.tol_adam(w0, G, *h, t0=t0, skip=skip, ref=r) for (w0, G, _, _, _), r in zip(inp, refs)]
    mirrors = [A.adam_fp32_mirror(w0, G, *h, t0=t0, skip=skip, form="kernel", hyper_f32=True, every_step=True) for w0, G, _, _, _ in inp]
    worst, bit_diff = [0.0, 0.0], [0, 0]
    applied = t0
    for k in range(K):
        gc, gf = inp[0][1][k], inp[1][1][k]
        if k in skip:                        # alternate the poisoned half
            if len([s for s in skip if s <= k]) % 2:
                gc = poisoned(gc)
            else:
                gf = poisoned(gf, value=float("-inf"))
            S.inject(ctx, gc, gf)
            with pytest.raises(NonFiniteGradientError):
                ctx.apply_adam()
        else:
            S.inject(ctx, gc, gf)
            ctx.apply_adam()
            applied += 1
        assert ctx.step == applied, (case, k)
        assert accumulator_is_zero(ctx), (case, k)
        if check_every_step or k == K - 1:
            for net in (0, 1):
                w = ctx.get_weights(net)
                err = float(np.abs(w - refs[net][k]).max())
                worst[net] = max(worst[net], err)
                assert err <= tols[net], (case, hyper, "step", k, "net", net, err, tols[net])
                w0, _, cls, _, _ = inp[net]
                assert np.array_equal(u32(w[cls == A.ZERO]), u32(w0[cls == A.ZERO])), (case, k, net, "always-zero class moved")
                bit_diff[net] = max(bit_diff[net], int(np.count_nonzero(u32(w) != u32(mirrors[net][k]))))
    return worst, tols, bit_diff


# ---- a. trajectory ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hyper", list(A.HYPER))
def test_trajectory_follows_fp64_adam(hyper):
    """12 injected steps, other schedules for the coarse and the fine half, every hyper-parameter set that reaches the GPU anywhere in
    the suite: after EVERY step both nets within tol_adam of float64 Keras-form Adam, the always-zero class bit-identical to w0, the
    accumulator exactly zero, the step count right.

    Measured on an MI355X: the weights equal the float32 mirror of adam_kernel (adam_reference.adam_fp32_mirror, form "kernel", lr_t
    from the float32 hyper-parameters the C ABI holds) in EVERY bit after every step, for all three sets (the build has no fast-math
    and -ffp-contract=off) -- asserted for the default set; the worst |w_gpu - fp64| is therefore that mirror's own, 1.24e-7 / 1.09e-7 /
    1.24e-7 against tol_adam 0.87e-6 ... 1.28e-6."""
    ctx = new_ctx(hyper)
    try:
        worst, tols, bit_diff = run_case(ctx, "trajectory", hyper)
        log_stats(f"optimizer_trajectory_{hyper}", worst_coarse=worst[0], worst_fine=worst[1], tol_coarse=tols[0], tol_fine=tols[1],
                  bits_differ_from_kernel_mirror_coarse=bit_diff[0], bits_differ_from_kernel_mirror_fine=bit_diff[1])
        print(f"\ntrajectory {hyper}: worst {worst}, tol_adam {tols}, elements that differ in bits from the kernel mirror {bit_diff}")
        if hyper == "default":
            assert bit_diff == [0, 0], bit_diff
    finally:
        ctx.close()


# ---- b. which half is which ---------------------------------------------------------------------------------------------------------

def test_a_gradient_in_one_half_moves_that_net_only():
    """[coarse | fine]: a gradient in the fine half leaves the coarse weights, the coarse query output and the coarse extended buffer
    (parameters + composed head) in their bits and moves the fine ones as the reference says; then the converse."""
    from keras_nerf_amd.debug import debug_buffer
    from tests.problem import make_problem
    P = make_problem(n_images=1, wh=4, weight_scale=1.0, bias_std=0.05)
    W = [O.flatten_params(P["cp"]), O.flatten_params(P["fp"])]
    h = A.HYPER["default"]
    rng = np.random.default_rng(9)
    pts = rng.uniform(-1.5, 1.5, (4096, 3)).astype(np.float32)
    dirs = rng.standard_normal((4096, 3)).astype(np.float32)
    G = [A.gradient_schedule(N, 1, 41)[0], A.gradient_schedule(N, 1, 42)[0]]
    for moving in (1, 0):                               # a fresh context each way: zero slots, so a zero gradient is no movement at all
        still = 1 - moving
        ctx = new_ctx(weights=W)
        try:
            def state(net):
                return (u32(ctx.get_weights(net)), S.bits(ctx.query_points(net, pts, dirs)),
                        S.bits(debug_buffer(ctx, 7, net).view(torch.float32)))
            before = state(still)
            q_before = S.bits(ctx.query_points(moving, pts, dirs))
            zero = np.zeros(N, np.float32)
            S.inject(ctx, *((zero, G[1][0]) if moving == 1 else (G[0][0], zero)))
            ctx.apply_adam()
            assert ctx.step == 1
            for name, x, y in zip(("weights", "query_points", "extended buffer"), before, state(still)):
                assert np.array_equal(x, y), ("net", still, name, "changed by a gradient in the other half")
            ref = A.adam_fp64(W[moving], G[moving], *h)
            tol = A.tol_adam(W[moving], G[moving], *h)
            err = float(np.abs(ctx.get_weights(moving) - ref).max())
            log_stats(f"optimizer_one_half_net{moving}", err=err, tol=tol)
            assert err <= tol, (moving, err, tol)
            assert not np.array_equal(S.bits(ctx.query_points(moving, pts, dirs)), q_before)
        finally:
            ctx.close()


# ---- c. skipped steps and the step count --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where,value", [(0, "nan"), (N - 1, "inf"), (N, "-inf"), (2 * N - 1, "nan"), (N, "inf"), (N - 1, "-inf")])
def test_finite_check_sees_the_whole_buffer(where, value):
    """first and last element of each half: both nets' weights keep their bits, the accumulator is cleared, the error is raised, the
    step count stays -- also after an applied step (slots non-zero), and the next good step is applied as if nothing had happened"""
    from keras_nerf_amd.runtime import NonFiniteGradientError
    h = A.HYPER["default"]
    G = [A.gradient_schedule(N, 2, 51)[0], A.gradient_schedule(N, 2, 52)[0]]
    w0 = [A.start_weights(N, s) for s in A.W0_SEEDS]
    ctx = new_ctx()
    try:
        S.inject(ctx, G[0][0], G[1][0]); ctx.apply_adam()
        before = [u32(ctx.get_weights(net)) for net in (0, 1)]
        both = np.concatenate([G[0][1], G[1][1]])
        both[where] = float(value)
        S.inject(ctx, both[:N], both[N:])
        with pytest.raises(NonFiniteGradientError):
            ctx.apply_adam()
        assert ctx.step == 1
        assert accumulator_is_zero(ctx)
        for net in (0, 1):
            assert np.array_equal(u32(ctx.get_weights(net)), before[net]), (net, where, value)
        ctx.poll_nonfinite(wait=True)                    # reported once
        S.inject(ctx, G[0][1], G[1][1]); ctx.apply_adam()
        assert ctx.step == 2
        for net in (0, 1):
            ref = A.adam_fp64(w0[net], G[net], *h)
            tol = A.tol_adam(w0[net], G[net], *h)
            assert np.abs(ctx.get_weights(net) - ref).max() <= tol, (net, where, value)
    finally:
        ctx.close()


def test_skipped_steps_touch_neither_slots_nor_t():
    """the trajectory with steps 4 and 9 poisoned = float64 Adam with those steps omitted, at every later step (a skipped step that
    advanced t would be off by 100 x tol_adam, tests/test_adam_host.py)"""
    ctx = new_ctx()
    try:
        worst, tols, _ = run_case(ctx, "skipped", "default")
        log_stats("optimizer_skipped_steps", worst_coarse=worst[0], worst_fine=worst[1], tol_coarse=tols[0], tol_fine=tols[1])
        assert ctx.step == 10
    finally:
        ctx.close()


def test_queued_steps_count_on_the_device():
    """three apply_adam(check=False) in a row with the gradients refilled in between on the same stream, the second one poisoned: the
    host learns of the skip only afterwards, so the THIRD step's t = 2 can only come from the device-side count.  One poll raises
    once, the next is clean, step == 2, weights = the reference with that step omitted."""
    from keras_nerf_amd.runtime import NonFiniteGradientError
    h = A.HYPER["default"]
    K, t0, skip = A.CASES["queued"]
    inp = [A.case_inputs("queued", net, N) for net in (0, 1)]
    ctx = new_ctx()
    try:
        dev = []
        for k in range(K):
            gc, gf = inp[0][1][k], inp[1][1][k]
            if k in skip:
                gf = poisoned(gf, where=N - 1, value=float("inf"))
            dev.append(torch.from_numpy(np.concatenate([gc, gf])).to(ctx.device))
        torch.cuda.synchronize()
        for k in range(K):                              # nothing below waits for the GPU
            ctx.grads_view().copy_(dev[k])
            ctx.apply_adam(check=False)
        with pytest.raises(NonFiniteGradientError):
            ctx.poll_nonfinite(wait=True)
        ctx.poll_nonfinite(wait=True)
        assert ctx.step == K - len(skip) == 2
        assert accumulator_is_zero(ctx)
        for net in (0, 1):
            w0, G, cls, _, _ = inp[net]
            ref = A.adam_fp64(w0, G, *h, t0=t0, skip=skip)
            tol = A.tol_adam(w0, G, *h, t0=t0, skip=skip)
            w = ctx.get_weights(net)
            err = float(np.abs(w - ref).max())
            log_stats(f"optimizer_queued_net{net}", err=err, tol=tol)
            assert err <= tol, (net, err, tol)
            assert np.array_equal(u32(w[cls == A.ZERO]), u32(w0[cls == A.ZERO]))
    finally:
        ctx.close()


def test_resume_from_a_step_count():
    """knerf_set_step_count is ABI for callers that resume a run (the Python package saves neither slots nor step and never calls it):
    step = 30 on a fresh context, six steps, the one of index 2 poisoned = float64 Adam with t0 = 30 and zero slots"""
    ctx = new_ctx()
    try:
        ctx.step = 30
        assert ctx.step == 30
        worst, tols, _ = run_case(ctx, "resume", "default")
        log_stats("optimizer_resume_t0_30", worst_coarse=worst[0], worst_fine=worst[1], tol_coarse=tols[0], tol_fine=tols[1])
        assert ctx.step == 35
        with pytest.raises(ValueError):
            ctx.step = -1
        assert ctx.step == 35
    finally:
        ctx.close()


# ---- d. derived state follows the fp32 masters, bit for bit;  e. the composed head against fp64 ------------------------------------

PRODUCT_SHAPES = [
    dict(),                                                         # 8 x 256 / 4
    dict(skip_layer=2),                                             # three concats, other stream tables
    dict(dense_units=128),
    dict(n_layers=4, dense_units=64, skip_layer=2),
    dict(dense_units=192),                                          # zero-padded to 256
    dict(force_generic=True, expect_fused=False),
    dict(n_layers=9, expect_fused=False),                           # the trunk ends in a concat; general-shape kernels in this library
]
XSHAPE_SPECS = ["9,4,256", "8,4,256,12,4"]      # fused, xshape library only: 63 more head rows (HeadOff with X = 63); other slot counts


def log_head(res):
    name = "optimizer_head_" + "_".join(str(v) for v in res["shape"]) + ("_generic" if res["force_generic"] else "")
    if res.get("fused"):
        (t0, e0), (t1, e1) = res["head_after_set_weights"], res["head_after_adam"]
        log_stats(name, tol_head_set_weights=t0, err_set_weights=e0, tol_head_adam=t1, err_adam=e1)
        print(f"\n{name}: after set_weights {e0:.3e} (tol_head {t0:.3e}), after apply_adam {e1:.3e} (tol_head {t1:.3e})")


@pytest.mark.parametrize("shape", PRODUCT_SHAPES, ids=lambda s: "-".join(f"{k}={v}" for k, v in s.items()) or "default")
def test_derived_state_is_the_same_by_every_route(shape):
    """tests/optimizer_state_check.py: apply_adam, set_weights and weights_view + refresh_weights lead to the same bits in query
    outputs, a rendered chunk, a deterministic train chunk's losses and whole gradient buffer (the only observer of the bf16 dgrad
    stream) and the extended weight buffer; all of them differ from the start weights'; set_weights of one net leaves the other
    alone; and on the fused shapes the composed head is within tol_head of float64 after set_weights and after the Adam steps."""
    log_head(S.run(**shape))


def test_derived_state_of_shapes_of_the_xshape_library():
    """the same body in a fresh process on the `xshape` build variant (tests/test_gpu_variants.py)"""
    from keras_nerf_amd import build as B
    from tests.variant_shapes import XSHAPES
    assert all(s in XSHAPES for s in XSHAPE_SPECS)
    lib = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "libknerf_hip_xshape.so")
    if not os.path.exists(lib):        # (where it exists, build() of __graft_entry__ has brought it up to date)
        lib = B.build(verbose=False, variant="xshape", add_shapes=XSHAPES)
    env = dict(os.environ, KNERF_LIB=lib, KNERF_PROBE_LIB=lib.replace("libknerf_hip_", "libknerf_probe_"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "optimizer_state_check.py")] + XSHAPE_SPECS, capture_output=True,
                       text=True, env=env, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [x["shape"] for x in rows] == [[9, 4, 256, 10, 4], [8, 4, 256, 12, 4]]
    for x in rows:
        assert x["fused"] is True
        log_head(x)
