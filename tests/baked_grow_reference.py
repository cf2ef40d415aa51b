"""NumPy reference of growing a baked field (include/knerf.h knerf_baked_train_tv / knerf_baked_resample), written from the
specification, not from the kernels: the total-variation regulariser over the slots of an optimiser with its gradient, the resampling
of a record table onto another lattice, and the regularised optimiser loop, coarse to fine, built from the functions of
tests/baked_train_reference.py.  Everything takes a dtype: float64 is the reference; float32 is the resampler's bit mirror (one rounding
per operation, as the kernel) and the optimiser's own rounding error (the tests' yardstick).
"""
import numpy as np

from tests import baked_train_reference as T


# ---- the record layout of include/knerf.h: fp32 sigma, 3 K halfs [k][c], zero padding to a multiple of 16 bytes
def record_bytes(degree):
    return (4 + 6 * (degree + 1) ** 2 + 15) // 16 * 16


def pack(sigma, coefficients, degree):
    """sigma [...] fp32, coefficients [..., K, 3] fp16 -> uint8 [P, record bytes]"""
    K = (degree + 1) ** 2
    sg = np.ascontiguousarray(sigma, dtype=np.float32).reshape(-1)
    co = np.ascontiguousarray(coefficients, dtype=np.float16).reshape(-1, 3 * K)
    rec = np.zeros((sg.size, record_bytes(degree)), dtype=np.uint8)
    rec[:, :4] = sg.view(np.uint8).reshape(-1, 4)
    rec[:, 4:4 + 6 * K] = co.view(np.uint8).reshape(-1, 6 * K)
    return rec


def unpack(records, degree):
    """(sigma [P] fp32, coefficients [P, K, 3] fp16); the padding is not looked at"""
    K = (degree + 1) ** 2
    rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, record_bytes(degree))
    return (np.ascontiguousarray(rec[:, :4]).view(np.float32).reshape(-1),
            np.ascontiguousarray(rec[:, 4:4 + 6 * K]).view(np.float16).reshape(-1, K, 3))


# ---- total variation over the slots
def tv_value_and_grad(master, slot_of, res, w_sigma, w_sh, eps, dtype=np.float64):
    """(R, grad [n_slots, W], (sum_p tv_sigma(p), sum_p sum_{q != sigma} tv_q(p))) of
        R = w_sigma sum_p tv_sigma(p) + w_sh sum_p sum_{q != sigma} tv_q(p),  tv_q(p) = sqrt(D_x^2 + D_y^2 + D_z^2 + eps),
    D_a q(p) = v_q(p + e_a) - v_q(p) where p + e_a lies in the lattice and has a slot, else 0.  master [n_slots, W] (sigma first),
    slot_of [points] (-1: no slot), res the lattice; all arithmetic in `dtype`.  The two sums are unweighted."""
    f = dtype
    w = np.asarray(master, dtype=f)
    n, W = w.shape
    slot = np.asarray(slot_of).reshape(res)
    has = slot >= 0
    V = np.zeros(tuple(res) + (W,), dtype=f)
    V[has] = w[slot[has]]
    D = []
    for a in range(3):
        nxt = np.zeros_like(V)
        nxt_has = np.zeros(res, dtype=bool)
        src = [slice(None)] * 3; dst = [slice(None)] * 3
        src[a], dst[a] = slice(1, None), slice(0, -1)
        nxt[tuple(dst)] = V[tuple(src)]
        nxt_has[tuple(dst)] = has[tuple(src)]
        both = has & nxt_has
        D.append(np.where(both[..., None], nxt - V, f(0)))
    tv = np.sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2] + f(eps))
    tv = np.where(has[..., None], tv, f(1))                               # outside the slots: never used, kept off the division
    weights = np.full(W, w_sh, dtype=f); weights[0] = f(w_sigma)
    terms = np.where(has[..., None], tv, f(0))
    sums = (float(terms[..., 0].sum(dtype=np.float64)), float(terms[..., 1:].sum(dtype=np.float64)))
    value = float(w_sigma) * sums[0] + float(w_sh) * sums[1]
    g = np.zeros_like(V)
    for a in range(3):
        ratio = np.where(has[..., None], D[a] / tv, f(0))                 # D_a(p) / tv(p); 0 where p has no successor with a slot
        g -= ratio
        src = [slice(None)] * 3; dst = [slice(None)] * 3
        src[a], dst[a] = slice(0, -1), slice(1, None)
        back = np.zeros_like(V)
        back[tuple(dst)] = ratio[tuple(src)]                              # D_a(p - e_a) / tv(p - e_a)
        g += back
    g = g * weights
    grad = np.zeros((n, W), dtype=f)
    grad[slot[has]] = g[has]
    return value, grad, sums


# ---- resampling onto another lattice
def placement(r, r_new):
    """(cell [r_new] int, f [r_new] float64): u = i (r - 1) / (r_new - 1) in double, cell = min(floor(u), r - 2), f = u - cell (the
    kernel rounds it to float32)"""
    i = np.arange(r_new, dtype=np.float64)
    u = i * np.float64(r - 1) / np.float64(r_new - 1)
    cell = np.minimum(np.floor(u), r - 2).astype(np.int64)
    return cell, u - cell


def _lerp(a, b, fr):
    one = fr.dtype.type(1)
    return a * (one - fr) + b * fr


def interpolate(values, res, res_new, dtype):
    """values [Rx,Ry,Rz,...] -> [R'x,R'y,R'z,...]: trilinear, z then y then x, each step a (1 - f) + b f with one rounding per operation
    in `dtype`; float32 rounds the fraction f to float32 first, float64 keeps it as it is"""
    v = np.asarray(values, dtype=dtype)
    extra = v.ndim - 3
    for axis in (2, 1, 0):
        cell, fr = placement(res[axis], res_new[axis])
        a, b = np.take(v, cell, axis=axis), np.take(v, cell + 1, axis=axis)
        shape = [1] * v.ndim
        shape[axis] = -1
        v = _lerp(a, b, fr.astype(dtype).reshape(shape))
        assert v.dtype == dtype
    assert v.ndim == 3 + extra
    return v


def corner_max(values, res, res_new):
    """max |value| over the 8 old corners every new point is interpolated from: the scale of its rounding error"""
    m = np.abs(np.asarray(values, dtype=np.float64))
    for axis in (2, 1, 0):
        cell, _ = placement(res[axis], res_new[axis])
        m = np.maximum(np.take(m, cell, axis=axis), np.take(m, cell + 1, axis=axis))
    return m


def resample(records, res, res_new, degree, threshold=0.0, dtype=np.float32):
    """(sigma [R'] dtype after the threshold, coefficients [R', K, 3] dtype BEFORE their rounding to fp16, records): the table on the
    lattice res_new.  sigma is interpolated from the fp32 values, a result <= fp32(threshold) is 0; the coefficients from the fp16
    values.  dtype float32: the kernel's arithmetic operation for operation, `records` are then its bytes (uint8 [P', record bytes],
    coefficients rounded to fp16 to nearest even, zero padding).  dtype float64: the yardstick; records is None."""
    sg, co = unpack(records, degree)
    K = (degree + 1) ** 2
    s = interpolate(sg.reshape(res), res, res_new, dtype)
    c = interpolate(co.reshape(tuple(res) + (K, 3)), res, res_new, dtype)
    s = np.where(s > dtype(np.float32(threshold)), s, dtype(0))
    rec = pack(s, c.astype(np.float16), degree) if dtype is np.float32 else None
    return s, c, rec


# ---- the regularised optimiser, coarse to fine
def slot_table(support):
    """(slots bool [points], slot_of int64 [points], trainable bool [n_slots]) of a support, slots ascending in lattice order"""
    slots = T.slot_points(support).reshape(-1)
    slot_of = np.full(slots.size, -1, dtype=np.int64)
    slot_of[slots] = np.arange(int(slots.sum()))
    return slots, slot_of, T.sigma_trainable(support).reshape(-1)[slots]


def optimise(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, lr_sigma, lr_sh, steps, tv_sigma=0.0, tv_sh=0.0,
             tv_epsilon=1e-6, dilation=0, beta_1=0.9, beta_2=0.999, epsilon=1e-7, white_background=False, termination=0.0,
             dtype=np.float64, order=None):
    """One stage: `steps` full-batch steps of tests/baked_train_reference.py's optimiser with the gradient of
    tv_sigma mean tv_sigma + tv_sh mean tv_q added before every Adam step (weights per term tv_sigma / n_slots and
    tv_sh / (3 K n_slots), rounded to fp32 as the launch takes them).  Returns (losses before every step, sigma fp32, coefficients fp16,
    master [n_slots, W] dtype): what the live field and the optimiser hold afterwards.  order: the ray order of the gradient sums."""
    sg = np.asarray(sigma, dtype=np.float32)
    co = np.asarray(coefficients, dtype=np.float16)
    res, K = sg.shape, co.shape[3]
    support = T.support_cells(sg, dilation)
    slots, slot_of, train = slot_table(support)
    n = int(slots.sum())
    w = np.concatenate([sg.reshape(-1, 1)[slots].astype(dtype) * train[:, None], co.reshape(-1, 3 * K)[slots].astype(dtype)], axis=1)
    m, v = np.zeros_like(w), np.zeros_like(w)
    ws, wc = float(np.float32(tv_sigma / n)), float(np.float32(tv_sh / (3.0 * K * n)))
    args = (lo, hi, origins, directions, near, far, step, target, support, white_background, termination)
    losses = []
    for t in range(1, steps + 1):
        L, gs, gc, _ = T.loss_and_grad(sg, co.astype(np.float64), *args, dtype=dtype, order=order)
        losses.append(L)
        g = np.concatenate([gs.reshape(-1, 1)[slots], gc.reshape(-1, 3 * K)[slots]], axis=1)
        if tv_sigma > 0 or tv_sh > 0:
            g = (g + tv_value_and_grad(w, slot_of, res, ws, wc, np.float32(tv_epsilon), dtype)[1]).astype(dtype)
        w, m, v, s32, c16 = T.adam_step(w, m, v, g, train, lr_sigma, lr_sh, beta_1, beta_2, epsilon, t, dtype=dtype)
        sg = sg.copy().reshape(-1); sg[slots] = s32; sg = sg.reshape(res)
        cf = co.copy().reshape(-1, 3 * K); cf[slots] = c16; co = cf.reshape(res + (K, 3))
    return losses, sg, co, w


def fit_coarse_to_fine(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, stages, lr_sigma, lr_sh, **kw):
    """stages [(resolution | None, steps), ...] as keras_nerf_amd.baked_train.fit_coarse_to_fine runs them: resample (the float32
    mirror, threshold 0), a fresh optimiser (moments from zero), `steps` steps, finish (sigma <= 0 is 0 already).  Returns (losses of
    all steps, the loss after the last step, sigma, coefficients)."""
    sg, co = np.asarray(sigma, dtype=np.float32), np.asarray(coefficients, dtype=np.float16)
    degree = int(round(np.sqrt(co.shape[3]))) - 1
    losses = []
    for resolution, steps in stages:
        if resolution is not None:
            s, _, rec = resample(pack(sg, co, degree), sg.shape, tuple(resolution), degree, 0.0, np.float32)
            sg, co = s.astype(np.float32), unpack(rec, degree)[1].reshape(tuple(resolution) + co.shape[3:])
        ls, sg, co, _ = optimise(sg, co, lo, hi, origins, directions, near, far, step, target, lr_sigma, lr_sh, steps, **kw)
        losses += ls
    final = T.loss_and_grad(sg, co.astype(np.float64), lo, hi, origins, directions, near, far, step, target, T.support_cells(sg),
                            kw.get("white_background", False), kw.get("termination", 0.0))[0]
    return losses, final, sg, co
