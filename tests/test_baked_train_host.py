"""Optimising a baked field, the parts that need no GPU: the NumPy reference's analytic gradient (tests/baked_train_reference.py)
against central differences of its own fp64 loss, the support / slot / trainable-sigma construction on a hand-made lattice, the Adam
step's masks, and the host-side argument checks of keras_nerf_amd/baked_train.py.

The finite-difference check pins the REFERENCE (the GPU tests compare the kernels with it).  Step and tolerance: the loss is smooth in
every parameter as long as no clamp gate and no termination cut flips inside [x - h, x + h]; the preconditions below keep every raw
colour, every output and every transmittance at least 1e-3 away from its kink, and a parameter moved by h = 1e-5 moves those by less
than 1e-4.  A central difference then has a truncation error of h^2 / 6 |L'''| (about 1e-11 for derivatives of order 1) and a
rounding error of 2^-53 L / h (about 1e-12 at L = 0.1); the largest gradient entries are 1e-3 .. 1e-2.  Tolerance: 1e-6 x the largest
entry of the tensor (about 1e-9 absolute, a hundred times the error estimate; a wrong term of the formula is off by the entry itself).
Measured: at most 2.1e-9 of the largest entry in every case (about 1e-11 absolute, the size of the estimate)."""
import numpy as np
import pytest

from tests import baked_train_reference as T

RES = (4, 4, 3)
LO, HI = (-1.0, -1.0, -0.6), (1.0, 1.0, 0.6)
STEP = 0.07
H = 1e-5


def _case(degree, seed=0, dense=1.0):
    rng = np.random.default_rng(40 + seed)
    K = (degree + 1) ** 2
    sigma = (rng.uniform(0.5, 3.0, RES) * dense).astype(np.float32)
    sigma[0:2, 0:2, :] = 0                                                 # two cells without density on any corner, and one more point
    sigma[3, 3, 2] = 0
    co = (rng.standard_normal(RES + (K, 3)) * 0.5).astype(np.float16)
    co[..., 0, :] += np.float16(1.6)
    n = 12
    lo, hi = np.array(LO), np.array(HI)
    o = 2.5 * (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.standard_normal((n, 3)))
    d = rng.uniform(lo * 0.8, hi * 0.8, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[3] *= 2.0                                                            # a direction that is no unit vector
    near, far = np.full(n, 0.2, dtype=np.float32), np.full(n, 5.0, dtype=np.float32)
    near[3], far[3] = 0.1, 2.5
    target = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    return sigma, co, o.astype(np.float32), d.astype(np.float32), near, far, target


@pytest.mark.parametrize("degree,white,termination,dense", [(0, False, 0.0, 1.0), (0, True, 0.0, 1.0), (2, False, 0.0, 1.0),
                                                            (2, True, 0.0, 1.0), (0, True, 0.05, 3.0), (2, False, 0.05, 3.0)])
def test_reference_gradient_matches_central_differences(degree, white, termination, dense):
    sigma, co, o, d, near, far, target = _case(degree, dense=dense)
    support = T.support_cells(sigma)
    assert support.any() and not support.all()
    co64 = co.astype(np.float64)
    args = (LO, HI, o, d, near, far, STEP, target, support, white, termination)
    info = {}
    L, gs, gc, _ = T.loss_and_grad(sigma.astype(np.float64), co64, *args, info=info)
    # preconditions: nothing sits on a kink, the colour clamp is exercised at degree 2, terminated rays exist where asked for
    raw, pre, Tn = info["raw"], info["pre"], info["T"]
    assert raw.shape[0] > 100
    assert np.abs(raw).min() > 1e-3 and np.abs(raw - 1).min() > 1e-3
    assert np.abs(pre).min() > 1e-3 and np.abs(pre - 1).min() > 1e-3
    if degree:
        assert ((raw < 0) | (raw > 1)).mean() > 0.01
    if termination:
        assert (Tn < termination).sum() >= 3 and np.abs(Tn / termination - 1).min() > 1e-2
    assert L > 1e-3 and np.abs(gs).max() > 0 and np.abs(gc).max() > 0
    rng = np.random.default_rng(5)
    worst = {"sigma": 0.0, "coef": 0.0}

    def loss(s, c):
        return T.loss_and_grad(s, c, *args)[0]
    s64 = sigma.astype(np.float64)
    for p in range(s64.size):                                             # every sigma, the points outside the slots included
        i = np.unravel_index(p, RES)
        a, b = s64.copy(), s64.copy()
        a[i] += H; b[i] -= H
        fd = (loss(a, co64) - loss(b, co64)) / (2 * H)
        worst["sigma"] = max(worst["sigma"], abs(fd - gs[i]))
    for p in rng.choice(co64.size, 40, replace=False):                    # and forty coefficients drawn at random
        i = np.unravel_index(p, co64.shape)
        a, b = co64.copy(), co64.copy()
        a[i] += H; b[i] -= H
        fd = (loss(s64, a) - loss(s64, b)) / (2 * H)
        worst["coef"] = max(worst["coef"], abs(fd - gc[i]))
    print(f"degree {degree} white {white} termination {termination}: max |fd - analytic| / max |g| = "
          f"{worst['sigma'] / np.abs(gs).max():.2e} (sigma), {worst['coef'] / np.abs(gc).max():.2e} (coefficients)")
    assert worst["sigma"] <= 1e-6 * np.abs(gs).max()
    assert worst["coef"] <= 1e-6 * np.abs(gc).max()
    slots = T.slot_points(support)
    assert np.all(gs[~slots] == 0) and np.all(gc[~slots] == 0)


def test_fp32_reference_and_ray_order():
    """the float32 form is the same function (its deviation is the GPU tests' yardstick) and the ray order only moves last bits"""
    sigma, co, o, d, near, far, target = _case(2)
    support = T.support_cells(sigma)
    args = (LO, HI, o, d, near, far, STEP, target, support, True, 0.0)
    L, gs, gc, out = T.loss_and_grad(sigma, co.astype(np.float64), *args)
    L32, gs32, gc32, out32 = T.loss_and_grad(sigma, co.astype(np.float64), *args, dtype=np.float32, order=np.arange(11, -1, -1))
    assert gs32.dtype == np.float32 and gc32.dtype == np.float32
    assert abs(L32 - L) < 1e-5 * L
    assert 0 < np.abs(gs32 - gs).max() < 1e-4 * np.abs(gs).max() and 0 < np.abs(gc32 - gc).max() < 1e-4 * np.abs(gc).max()
    # half batches normalised by the whole count add up to the whole batch
    h1 = T.loss_and_grad(sigma, co.astype(np.float64), LO, HI, o[:6], d[:6], near[:6], far[:6], STEP, target[:6], support, True, 0.0, n_norm=12)
    h2 = T.loss_and_grad(sigma, co.astype(np.float64), LO, HI, o[6:], d[6:], near[6:], far[6:], STEP, target[6:], support, True, 0.0, n_norm=12)
    assert np.allclose(h1[1] + h2[1], gs, rtol=0, atol=1e-14) and np.allclose(h1[2] + h2[2], gc, rtol=0, atol=1e-14)
    assert abs(h1[0] + h2[0] - L) < 1e-14


def test_support_slots_and_trainable_sigma():
    """one dense point in a 6 x 5 x 5 lattice: its 8 cells are the support, their 27 corners the slots, and only the point itself has
    all 8 adjacent cells in the support; dilation grows both sets"""
    sigma = np.zeros((6, 5, 5), dtype=np.float32)
    sigma[2, 2, 2] = 1.0
    sup = T.support_cells(sigma)
    assert sup.sum() == 8 and sup[1:3, 1:3, 1:3].all()
    slots, train = T.slot_points(sup), T.sigma_trainable(sup)
    assert slots.sum() == 27 and slots[1:4, 1:4, 1:4].all()
    assert train.sum() == 1 and train[2, 2, 2]
    assert slots[1, 2, 2] and not train[1, 2, 2]                        # a boundary point: a slot, its sigma fixed at 0
    sup1 = T.support_cells(sigma, 1)
    slots1, train1 = T.slot_points(sup1), T.sigma_trainable(sup1)
    assert sup1.sum() == 4 * 4 * 4 and sup1[0:4].all() and not sup1[4].any()        # y and z are covered entirely, x is not
    assert slots1.sum() == 5 * 5 * 5 and (slots1 >= slots).all() and slots1.sum() > slots.sum()
    # along x the points 0..3 have both neighbours in the support (or outside the lattice), point 4 borders cell 4; y, z: all covered
    assert train1[0:4].all() and not train1[4:].any() and (train1 >= train).all() and train1.sum() > train.sum()
    # a corner point at the lattice's edge: cells outside the lattice do not count against it
    sigma = np.zeros((3, 3, 3), dtype=np.float32)
    sigma[0, 0, 0] = 2.0
    sup = T.support_cells(sigma)
    assert sup.sum() == 1 and T.slot_points(sup).sum() == 8
    assert T.sigma_trainable(sup).sum() == 1 and T.sigma_trainable(sup)[0, 0, 0]
    # the invariant the construction is for: every cell outside the support has no trainable sigma on any corner
    rng = np.random.default_rng(3)
    sigma = rng.uniform(0, 1, (7, 6, 5)).astype(np.float32) * (rng.random((7, 6, 5)) < 0.15)
    for dil in (0, 1, 2):
        sup = T.support_cells(sigma, dil)
        train = T.sigma_trainable(sup)
        assert (train <= T.slot_points(sup)).all()
        assert (sigma[~train] == 0).all()                                # a point beside a cell outside the support has no density
        corners = np.zeros(sup.shape, dtype=bool)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    corners |= train[a:a + sup.shape[0], b:b + sup.shape[1], c:c + sup.shape[2]]
        assert not (corners & ~sup).any()


def test_adam_step_masks_projects_and_repacks():
    rng = np.random.default_rng(1)
    n, W = 50, 1 + 3 * 4
    w = rng.normal(0, 0.5, (n, W)); w[:, 0] = np.abs(w[:, 0])
    train = rng.random(n) < 0.5
    w[~train, 0] = 0
    g = rng.normal(0, 1e-2, (n, W)); g[:, 0] = np.abs(g[:, 0]) * 50          # pushes sigma down hard: the projection acts
    m, v = np.zeros_like(w), np.zeros_like(w)
    w1, m1, v1, s32, c16 = T.adam_step(w, m, v, g, train, 0.5, 1e-2, 0.9, 0.999, 1e-7, 1)
    # from zero moments the first Keras-form step is lr g / (|g| + eps / sqrt(1 - b2)): the bias corrections cancel
    first = lambda lr, x: lr * x / (np.abs(x) + 1e-7 / np.sqrt(1 - 0.999))
    assert np.allclose(w1[:, 1:], w[:, 1:] - first(1e-2, g[:, 1:]), rtol=0, atol=1e-14)
    assert np.allclose(w1[train, 0], np.maximum(w[train, 0] - first(0.5, g[train, 0]), 0), rtol=0, atol=1e-14)
    assert (w1[:, 0] >= 0).all() and (w1[train, 0] == 0).any() and (w1[train, 0] > 0).any()
    assert (w1[~train, 0] == 0).all() and (m1[~train, 0] == 0).all() and (v1[~train, 0] == 0).all()
    assert s32.dtype == np.float32 and c16.dtype == np.float16 and np.array_equal(c16, w1[:, 1:].astype(np.float16))
    w32 = T.adam_step(w, m, v, g, train, 0.5, 1e-2, 0.9, 0.999, 1e-7, 1, dtype=np.float32)[0]
    assert w32.dtype == np.float32 and np.abs(w32 - w1).max() < 1e-5
    # step 3 of a run uses the bias correction of t = 3
    w3 = T.adam_step(w1, m1, v1, g, train, 0.5, 1e-2, 0.9, 0.999, 1e-7, 3)[0]
    corr = np.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)
    m3, v3 = 0.9 * m1 + 0.1 * g, 0.999 * v1 + 0.001 * g * g
    assert np.allclose(w3[:, 1:], w1[:, 1:] - 1e-2 * corr * m3[:, 1:] / (np.sqrt(v3[:, 1:]) + 1e-7), rtol=0, atol=1e-15)


def test_argument_validation():
    from keras_nerf_amd import baked
    from keras_nerf_amd.baked_train import check_optimizer_args, check_target_shape, bias_corrected_rate
    assert baked.BakedFieldOptimizer is not None and baked.check_optimizer_args is check_optimizer_args
    assert check_optimizer_args(1.0, 1e-2, 0.9, 0.999, 1e-7, 0) == (1.0, 1e-2, 0.9, 0.999, 1e-7, 0)
    assert check_optimizer_args(1, 1, 0.0, 0.0, 1.0, 8)[5] == 8
    good = dict(learning_rate_sigma=1.0, learning_rate_sh=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dilation=0)
    for key, bad in (("learning_rate_sigma", 0.0), ("learning_rate_sigma", -1.0), ("learning_rate_sigma", float("nan")),
                     ("learning_rate_sh", 0.0), ("learning_rate_sh", float("inf")), ("learning_rate_sh", "1e-2"),
                     ("beta_1", 1.0), ("beta_1", -0.1), ("beta_2", 1.0), ("beta_2", 1.5), ("epsilon", 0.0), ("epsilon", -1e-7),
                     ("epsilon", 1e-60), ("dilation", -1), ("dilation", 9), ("dilation", 1.5), ("dilation", True)):
        with pytest.raises(ValueError, match=key.split("_")[0]):
            check_optimizer_args(**{**good, key: bad})
    check_target_shape((7, 3), 7)
    for shape in ((7,), (7, 4), (6, 3), (7, 3, 1), (3, 7)):
        with pytest.raises(ValueError, match="target"):
            check_target_shape(shape, 7)
    assert bias_corrected_rate(1e-3, 0.9, 0.999, 1) == pytest.approx(1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9), rel=1e-15)
    assert bias_corrected_rate(1e-3, 0.0, 0.0, 5) == 1e-3


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID in the style of knerf_baked_render, decided on the host: no device is needed"""
    import ctypes as C
    from keras_nerf_amd import _lib
    lib = _lib.load()
    INV = _lib.KNERF_ERR_INVALID
    p = C.c_void_p(4096)                                                  # never dereferenced: every call below is refused first

    def state(res=(9, 7, 6), degree=2, lo=(-1.0,) * 3, hi=(1.0,) * 3, records=p, bits=p, slot_of=p, grad=p, n_slots=10):
        f = _lib.KnerfBakedField(records, bits, (C.c_int32 * 3)(*res), degree, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi))
        return _lib.KnerfBakedTrain(f, slot_of, grad, n_slots)

    def rays(st, o=p, d=p, target=p, n=10, n_norm=0, step=0.05, term=0.0, flags=0):
        return lib.knerf_baked_train_rays(None, C.byref(st) if st is not None else None, o, d, None, None, 0.0, 1.0, target, n, n_norm,
                                          step, term, flags, None)

    def apply(st, point_of=p, train=p, w=p, m=p, v=p, rs=0.1, rc=0.01, b1=0.9, b2=0.999, eps=1e-7):
        return lib.knerf_baked_train_apply(None, C.byref(st) if st is not None else None, point_of, train, w, m, v, rs, rc, b1, b2, eps)

    assert rays(state(), n=0) == 0                                        # no rays: nothing to launch
    for call in (rays, apply):
        assert call(None) == INV
        for bad in (dict(records=None), dict(bits=None), dict(slot_of=None), dict(grad=None), dict(degree=4), dict(degree=-1),
                    dict(res=(1, 7, 6)), dict(res=(9, 1026, 6)), dict(hi=(1.0, -1.0, 1.0)), dict(lo=(float("nan"), -1.0, -1.0)),
                    dict(n_slots=0), dict(n_slots=9 * 7 * 6 + 1)):
            assert call(state(**bad)) == INV, (call.__name__, bad)
    for bad in (dict(o=None), dict(d=None), dict(target=None), dict(step=0.0), dict(step=float("inf")), dict(term=1.0), dict(term=-0.1),
                dict(flags=4), dict(flags=2 << 8), dict(n=1 << 36), dict(n_norm=1 << 36)):
        assert rays(state(), **bad) == INV, bad
    assert rays(state(degree=0), flags=4 << 8) == INV and rays(state(degree=1), flags=4 << 8) == INV      # lane counts the degree lacks
    assert rays(state(degree=3), flags=2 << 8) == INV
    for bad in (dict(point_of=None), dict(train=None), dict(w=None), dict(m=None), dict(v=None), dict(rs=float("nan")),
                dict(rc=float("inf")), dict(b1=1.0), dict(b2=-0.1), dict(eps=0.0)):
        assert apply(state(), **bad) == INV, bad


def defined_once_in_the_header(heads):
    """every head of `heads` is defined exactly once across csrc/baked*.hip and csrc/baked_common.h, and that once is in the header; every
    baked*.hip that calls one of them includes the header"""
    import glob
    import os
    import re
    from keras_nerf_amd import baked
    csrc = os.path.join(os.path.dirname(os.path.abspath(baked.__file__)), "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "baked*.hip")))
    assert len(files) >= 5, files
    text = {os.path.basename(f): re.sub(r"//[^\n]*", "", open(f).read()) for f in files + [os.path.join(csrc, "baked_common.h")]}
    for head in heads:
        where = [(name, src.count(head)) for name, src in text.items() if head in src]
        assert where == [("baked_common.h", 1)], (head, where)
    for name, src in text.items():
        if name == "baked_common.h":
            continue
        calls = [head for head in heads if re.search(r"\b" + re.escape(head.split()[-1].rstrip("(")) + r"\s*[<(]", src)]
        assert not calls or '#include "baked_common.h"' in src, (name, calls)


# the definitions' first lines as they stand in the header (template heads are on the line above)
MARCH_HELPERS = ("__device__ __forceinline__ void sh_eval(", "__device__ __forceinline__ float group_sum(",
                 "__device__ __forceinline__ float group_first(", "__device__ __forceinline__ bool locate(",
                 "__device__ __forceinline__ float dpp(", "__host__ __device__ constexpr int n_coeff(",
                 "__host__ __device__ constexpr int rec_bytes(", "__device__ __forceinline__ float half_bits_to_float(")


def test_the_march_helpers_are_defined_once_in_the_shared_header():
    """sh_eval, the DPP group sums, locate and the record's sizes and codec: one definition, in csrc/baked_common.h, for every baked*.hip"""
    defined_once_in_the_header(MARCH_HELPERS)
