"""What the tolerances of tests/test_gpu_optimizer.py rest on, proved on the CPU (no GPU needed) for exactly the inputs, cases and
hyper-parameter sets that file uses (tests/adam_reference.py CASES / HYPER / GPU_RUNS):

* tolerance: tol_adam = 8 x the worst error of the two float32 mirrors against float64 Adam on the very schedule -- computed at run
  time from NumPy alone, never from GPU output;
* power: each of the ten deliberately wrong Adams differs from the float64 reference by more than 10 x tol_adam in max-norm, so a
  kernel that made one of those mistakes could not pass;
* the always-zero class keeps the bits of w0 in both mirrors;
* the composed head: the float32 mirror in head_compose_kernel's loop order against oracle.head_compose in float64.

Measured (595,844 elements per net, the worse net): mirror error 1.6e-7 (defaults, 12 steps), 1.1e-7 (lr 5e-4), 1.2e-7 (lr 2e-4,
betas 0.8 / 0.99), 1.6e-7 (12 steps, two skipped), 4.7e-8 (3 steps, one skipped), 8.1e-8 (6 steps from t0 = 30, one skipped).  Weakest
mutants, as multiples of tol_adam (= 8 x that error): "skipped step advances t" 54 (resume from t0 = 30), 100 (two skips in 12
steps), 380 (3 queued steps); t + 1: 78 (t0 = 30), 94 (betas 0.8 / 0.99), 370 ... 1,200 elsewhere; every other >= 600.  The printed
table (pytest -s) has every figure."""
import numpy as np
import pytest

from oracle import nerf_oracle as O
from tests import adam_reference as A
from tests.problem import make_problem

N = O.param_count(O.NerfConfig())          # 595,844: not a multiple of 256, the last Adam workgroup is partial


def test_the_default_shape_has_a_partial_last_workgroup():
    assert N == 595844 and N % 256 != 0


def test_schedule_classes_and_cap():
    G, cls = A.gradient_schedule(50_000, 5, 3)
    assert all(g.dtype == np.float32 and g.shape == (50_000,) for g in G)
    share = [float(np.mean(cls == c)) for c in (A.ZERO, A.FIRST_ONLY, A.CONST_SIGN)]
    assert all(0.04 < s < 0.06 for s in share), share
    assert all(not g[cls == A.ZERO].any() for g in G)
    assert G[0][cls == A.FIRST_ONLY].any() and all(not g[cls == A.FIRST_ONLY].any() for g in G[1:])
    assert all((g[cls == A.CONST_SIGN] >= 0).all() for g in G)
    zeros = float(np.mean(G[2][cls == A.FREE] == 0))
    assert 0.18 < zeros < 0.22, zeros
    mx = max(float(np.abs(g).max()) for g in G)
    assert mx <= A.G_CAP and np.isfinite(np.float32(mx) * np.float32(mx))
    mags = np.abs(G[0][G[0] != 0])
    assert mags.min() < 1e-11 and mags.max() > 1e2          # the whole range on both sides of epsilon


def test_fp64_reference_is_the_oracles_keras_adam():
    rng = np.random.default_rng(0)
    w0 = rng.normal(0, 0.1, 4096)
    G = [rng.standard_normal(4096) for _ in range(5)]
    p = [w0.copy()]
    opt = O.KerasAdam(p, lr=5e-4, b1=0.8, b2=0.99, eps=1e-8)
    for g in G:
        opt.apply(p, [g])
    np.testing.assert_allclose(A.adam_fp64(w0, G, 5e-4, 0.8, 0.99, 1e-8), p[0], rtol=0, atol=1e-15)
    # a skipped step is no step at all; t0 shifts the bias correction only
    np.testing.assert_array_equal(A.adam_fp64(w0, G, 1e-3, 0.9, 0.999, 1e-7, skip=(1, 3)),
                                  A.adam_fp64(w0, [G[0], G[2], G[4]], 1e-3, 0.9, 0.999, 1e-7))
    assert np.abs(A.adam_fp64(w0, G, 1e-3, 0.9, 0.999, 1e-7, t0=30) - A.adam_fp64(w0, G, 1e-3, 0.9, 0.999, 1e-7)).max() > 1e-5


@pytest.mark.parametrize("case,hyper", A.GPU_RUNS)
def test_tolerance_power_and_exact_zeros(case, hyper):
    h = A.HYPER[hyper]
    for net in (0, 1):
        w0, G, cls, t0, skip = A.case_inputs(case, net, N)
        ref = A.adam_fp64(w0, G, *h, t0=t0, skip=skip, every_step=True)
        err = A.mirror_error(w0, G, *h, t0=t0, skip=skip, ref=ref)
        tol = A.TOL_FACTOR * err
        print(f"\n{case:10s} {hyper:10s} net {net}: K {len(G)} t0 {t0} skip {skip}  mirror error {err:.3e}  tol_adam {tol:.3e}")
        assert 0 < tol < 1e-2 * h[0]                       # far below one step's movement (lr)
        for m in A.mutants_for(skip):
            d = float(np.abs(A.adam_fp64(w0, G, *h, t0=t0, skip=skip, mutant=m) - ref[-1]).max())
            print(f"    {m:20s} max |mutant - fp64| {d:.3e} = {d / tol:9.1f} x tol_adam")
            assert d > A.POWER_FACTOR * tol, (case, hyper, net, m, d, tol)
        for form in ("kernel", "keras"):
            w = A.adam_fp32_mirror(w0, G, *h, t0=t0, skip=skip, form=form)
            assert np.array_equal(w[cls == A.ZERO].view(np.uint32), w0[cls == A.ZERO].view(np.uint32))
            assert (w[cls != A.ZERO] != w0[cls != A.ZERO]).mean() > 0.5       # (gradients far below epsilon move less than an ulp)


def test_late_steps_hide_the_step_count():
    """why the resume case starts at t0 = 30 and not at a large count: lr_t flattens, and at t0 = 5000 a wrong t is invisible"""
    h = A.HYPER["default"]
    w0, G, cls, _, skip = A.case_inputs("resume", 0, 100_000)
    ref = A.adam_fp64(w0, G, *h, t0=5000, skip=skip)
    tol = A.tol_adam(w0, G, *h, t0=5000, skip=skip)
    for m in ("skip_advances_t", "t_plus_1"):
        assert np.abs(A.adam_fp64(w0, G, *h, t0=5000, skip=skip, mutant=m) - ref).max() < tol


@pytest.mark.parametrize("units,scale,nl,sk", [(256, 1.0, 8, 4), (256, 1.5, 8, 4), (64, 1.0, 8, 4), (256, 1.5, 9, 4)])
def test_head_mirror_against_fp64(units, scale, nl, sk):
    cfg = O.NerfConfig(dense_units=units, n_layers=nl, skip_layer=sk)
    P = make_problem(n_images=1, wh=4, weight_scale=scale, bias_std=0.05, cfg=cfg)
    for params in (P["cp"], P["fp"]):
        H64, H32 = A.head_fp64(params, cfg), A.head_fp32_mirror(params, cfg)
        Tr, D, rows = A.head_layout(cfg)
        assert H64.size == rows * 4 + 4 == H32.size
        tol = A.tol_head(params, cfg)
        print(f"\nhead {nl}x{units}/{sk} scale {scale}: max |H| {np.abs(H64).max():.3f}  mirror error {tol / A.TOL_FACTOR:.3e}  tol_head {tol:.3e}")
        assert 0 < tol < 1e-5 * np.abs(H64).max()
        M = H32[:rows * 4].reshape(rows, 4)
        assert not M[Tr + D:].any() and not M[Tr:, 3].any()                          # padding rows, sigma column of the direction rows
        n = cfg.n_layers
        assert np.array_equal(M[:Tr, 3], params[2 * n][:, 0]) and H32[-1] == params[2 * n + 1][0]    # the sigma column is a copy
        # a head composed from the OTHER net's weights is far outside the tolerance
    other = A.head_fp64(P["fp"], cfg)
    assert np.abs(A.head_fp32_mirror(P["cp"], cfg) - other).max() > 1e3 * A.tol_head(P["cp"], cfg)


def test_head_layout_of_the_shapes_the_gpu_test_uses():
    assert A.head_layout(O.NerfConfig()) == (256, 27, 288)                                  # layout.h: DefaultShape::kHeadRows == 288
    assert A.head_layout(O.NerfConfig(n_layers=9)) == (319, 27, 256 + 64 + 32)              # the trunk ends in a concat: 63 more rows
    assert A.head_layout(O.NerfConfig(pos_emb_xyz=12, pos_emb_dir=4)) == (256, 27, 288)
    assert A.head_layout(O.NerfConfig(n_layers=4, dense_units=64, skip_layer=2)) == (64, 27, 96)
    assert A.enc_slots(8) == 64 and A.enc_slots(6) == 64 and A.enc_slots(1) == 32
