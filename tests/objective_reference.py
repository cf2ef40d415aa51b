"""NumPy references for csrc/composite_ext.hip -- the compositing kernel with an extended objective (include/knerf.h
knerf_set_objective): mae / huber / log-cosh photometric terms, the distortion and the opacity-entropy regulariser.  Built on
tests/composite_reference.py (CR): its inputs and ray classes, its float32-elementwise / float64-cumulative reference, its mirror of
the kernel's structure, its jittered exp, its rule for undecidable clip gates, its error measures and its two factors.

reference()  CR.reference extended by the objective; the distortion term in its PREFIX form in float64 (tests/test_objective_host.py
             ties that form to the O(S^2) definition under float64 autograd).  Returns the four terms and the workgroups' partials too.
mirror32()   composite_ext_kernel<C> in float32 NumPy, operation by operation.  The device's logf / log1pf / tanhf are not NumPy's: the
             `jitter` variant moves every result of exp, log, log1p and tanh one ulp up or down at random, as CR.exp_jittered does.
case()       inputs (CR.case's), reference, the rays left out of the gated comparisons and tolerances = 8 x the mirror's error.
MUTANTS      the reference with one mistake each.

Left out of the gated comparisons (draw, the last sample's dsigma): rays whose clip gate is undecidable (CR.undecidable); with the
entropy weight set, rays whose acc lies within 1e-5 of a clamp bound (the gate of dH/dw); with the distortion weight set, the class
UNSORTED (the contract is non-decreasing t; the kernel returns the prefix form's value there, and the outputs must be finite).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import composite_reference as CR

F = np.float32
MSE, MAE, HUBER, LOG_COSH = 0, 1, 2, 3
ACC_LO, ACC_HI = F(1e-4), F(1.0) - F(1e-4)         # the entropy clamp, the kernel's float32 constants
ACC_EDGE = 1e-5
TERMS = ("photometric", "mse", "distortion", "opacity_entropy")

# name -> (kind, huber_delta, distortion, opacity_entropy); tests/test_gpu_objective.py runs every one of them on every S below
OBJECTIVES = {
    "mae": (MAE, 0.0, 0.0, 0.0),
    "huber": (HUBER, 0.25, 0.0, 0.0),              # |d| lies between 0.05 and 1: both branches occur
    "log_cosh": (LOG_COSH, 0.0, 0.0, 0.0),
    "mse_distortion": (MSE, 0.0, 0.01, 0.0),
    "mse_entropy": (MSE, 0.0, 0.0, 0.001),
    "huber_both": (HUBER, 0.25, 0.01, 0.001),
}
PLAIN = (MSE, 0.0, 0.0, 0.0)
S_CASES = (2, 5, 64, 65, 192, 250, 257, 513, 1024)      # one S per template C (1, 2, 3, 4, 8, 12, 16) plus the ragged ones
TILE_S = (32, 192, 1024)

MUTANTS = ("mae_sign_of_zero_is_one", "huber_linear_branch_unclamped", "huber_quadratic_everywhere", "logcosh_grad_is_d",
           "reg_through_clip_gate", "dist_without_self_term", "dist_prefix_inclusive", "dist_one_sided", "dist_midpoint_is_t",
           "entropy_gate_dropped", "entropy_sign_flipped", "reg_scale_missing", "regs_on_wrong_net")


def rho64(kind, delta, d):
    """(rho(d), rho'(d) / 2) in float64"""
    a = np.abs(d)
    if kind == MAE:
        return a, 0.5 * np.sign(d)
    if kind == HUBER:
        return np.where(a <= delta, 0.5 * d * d, delta * (a - 0.5 * delta)), 0.5 * np.clip(d, -delta, delta)
    if kind == LOG_COSH:
        return a + np.log1p(np.exp(-2.0 * a)) - np.log(2.0), 0.5 * np.tanh(d)
    return d * d, d


def regularizers64(w, m, delta, mutant=None):
    """per ray D, H and per sample dD/dw, dH/dw in float64 from the weights, the midpoints (relative to t_0) and the intervals:
    the prefix form, which equals the O(S^2) definition for non-decreasing m"""
    wm = w * m
    W, M = np.cumsum(w, axis=1), np.cumsum(wm, axis=1)
    Wt, Mt = W[:, -1:], M[:, -1:]
    # exclusive prefix sums.  (The mutant takes W alone inclusively: with BOTH sums inclusive the sample's own term is
    # w_k (m_k - m_k) = 0 and nothing changes -- that variant is no mistake and cannot be told apart.)
    W, M = (W if mutant == "dist_prefix_inclusive" else W - w), M - wm
    Ws, Ms = (Wt - W) - w, (Mt - M) - wm                           # exclusive suffix sums: the total less the prefix less the sample
    before = m * W - M
    self_d, self_g = (1.0 / 3.0) * w * w * delta, (2.0 / 3.0) * w * delta
    if mutant == "dist_without_self_term":
        self_d, self_g = 0.0 * self_d, 0.0 * self_g
    D = (2.0 * w * before + self_d).sum(axis=1)
    gD = 2.0 * (before + ((Ms - m * Ws) if mutant != "dist_one_sided" else 0.0)) + self_g
    acc = w.sum(axis=1)
    lo, hi = float(ACC_LO), float(ACC_HI)
    a = np.clip(acc, lo, hi)
    H = -a * np.log(a) - (1.0 - a) * np.log(1.0 - a)
    inside = (acc >= lo) & (acc <= hi)
    dH = np.log((1.0 - a) / a)
    if mutant != "entropy_gate_dropped":
        dH = np.where(inside, dH, 0.0)
    if mutant == "entropy_sign_flipped":
        dH = -dH
    return D, H, gD, dH


def wg_partials(per_ray):
    """the workgroups' sums (four rays each) of per-ray terms [..., R] -> [..., ceil(R/4)] in float64"""
    p = np.concatenate([per_ray, np.zeros(per_ray.shape[:-1] + (-per_ray.shape[-1] % 4,))], axis=-1)
    return p.reshape(per_ray.shape[:-1] + (-1, 4)).sum(axis=-1)


# ------------------------------------------------------------------------------------------------------------- reference
def reference(raw, t, target, white, grad_scale, loss_scale, reg_scale, objective, net=0, nets=3, own_pixel=None, loss0=0.0, mutant=None):
    """dict(image, pre, depth, weights, draw, loss, terms [4], partial [ceil(R/4)], terms_partial [4, ceil(R/4)], acc) in float64.
    objective = (kind, huber_delta, distortion, opacity_entropy); the regularisers apply when bit `net` of `nets` is set."""
    assert mutant is None or mutant in MUTANTS, mutant
    kind, hd, lam_d, lam_e = objective
    on = (nets >> ((1 - net) if mutant == "regs_on_wrong_net" else net)) & 1
    lam_d, lam_e = (lam_d, lam_e) if on else (0.0, 0.0)
    ft = raw.dtype.type
    R, S = t.shape
    rgb, sigma = raw[..., :3].astype(np.float64), raw[..., 3]
    eps = ft(1e-10)
    delta = np.concatenate([t[:, 1:] - t[:, :-1], np.full((R, 1), eps, raw.dtype)], axis=-1)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        ex = np.exp(-(sigma * delta).astype(np.float64)).astype(raw.dtype)
        alpha = ft(1.0) - ex
        x = (ft(1.0) - alpha) + eps
        delta, ex, alpha, x = (v.astype(np.float64) for v in (delta, ex, alpha, x))
        T = np.cumprod(x, axis=-1)
        T = np.concatenate([np.ones((R, 1)), T[:, :-1]], axis=-1)
        w = alpha * T
        pre = np.sum(w[..., None] * rgb, axis=1)
        if white:
            pre = pre + (1.0 - np.sum(w, axis=-1))[:, None]
        image = np.clip(pre, 0.0, 1.0)
        t64 = t.astype(np.float64)
        depth = np.sum(w * t64, axis=-1)
        tgt = target.astype(np.float64).copy()
        if own_pixel is not None:
            tgt[own_pixel] = image[own_pixel]
        df = image - tgt
        rho, h = rho64(kind, hd, df)
        if mutant == "mae_sign_of_zero_is_one" and kind == MAE:
            h = np.where(df >= 0, 0.5, -0.5)
        if mutant in ("huber_linear_branch_unclamped", "logcosh_grad_is_d") and kind == (HUBER if mutant.startswith("huber") else LOG_COSH):
            h = 0.5 * df
        if mutant == "huber_quadratic_everywhere" and kind == HUBER:
            rho = 0.5 * df * df
        gate = (pre >= 0.0) & (pre <= 1.0)
        g = np.where(gate, grad_scale * h, 0.0)
        dw = np.sum(rgb * g[:, None, :], axis=-1)
        if white:
            dw = dw - np.sum(g, axis=-1)[:, None]
        m = (t64 - t64[:, :1]) + (0.0 if mutant == "dist_midpoint_is_t" else 0.5 * delta)
        D, H, gD, dH = regularizers64(w, m, delta, mutant)
        if lam_d != 0 or lam_e != 0:
            reg = (1.0 if mutant == "reg_scale_missing" else reg_scale) * (lam_d * gD + lam_e * dH[:, None])
            if mutant == "reg_through_clip_gate":
                reg = reg * gate.all(axis=1)[:, None]
            dw = dw + reg
        prod = dw * w
        Q = np.zeros((R, S))
        Q[:, :-1] = np.cumsum(prod[:, :0:-1], axis=-1)[:, ::-1]
        dalpha = dw * T - Q / x
        dsigma = dalpha * delta * ex
        draw = np.concatenate([w[..., None] * g[:, None, :], dsigma[..., None]], axis=-1)
        per_ray = np.stack([loss_scale * rho.sum(axis=1), loss_scale * (df * df).sum(axis=1), reg_scale * D, reg_scale * H])
        ray_loss = per_ray[0] + lam_d * per_ray[2] + lam_e * per_ray[3]
    return dict(image=image, pre=pre, depth=depth, weights=w, draw=draw, loss=float(loss0 + ray_loss.sum()), terms=per_ray.sum(axis=1),
                partial=wg_partials(ray_loss), terms_partial=wg_partials(per_ray), acc=w.sum(axis=1))


# ---------------------------------------------------------------------------------------------------------------- mirror
def _jittered(fn, rng):
    def f(a):
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            e = fn(a).astype(F)
        up = rng.random(a.shape) < 0.5
        j = np.nextafter(e, np.where(up, F(np.inf), F(-np.inf)).astype(F))
        keep = (e == 1) | (e == 0) | ~np.isfinite(e)
        return np.where(keep, e, j).astype(F)
    return f


def math_numpy():
    return dict(exp=CR.exp_numpy, log=np.log, log1p=np.log1p, tanh=np.tanh)


def math_jittered(seed):
    rng = np.random.default_rng(seed)
    return dict(exp=CR.exp_jittered(seed), log=_jittered(np.log, rng), log1p=_jittered(np.log1p, rng), tanh=_jittered(np.tanh, rng))


def _scan_add_exclusive(v):
    """six __shfl_up steps of an inclusive sum over the 64 lanes, then one lane down with 0 in lane 0"""
    inc = v
    for o in (1, 2, 4, 8, 16, 32):
        new = inc.copy()
        new[:, o:] = inc[:, o:] + inc[:, :-o]
        inc = new
    out = np.zeros_like(v)
    out[:, 1:] = inc[:, :-1]
    return out


def mirror32(raw, t, target, white, grad_scale, loss_scale, reg_scale, objective, own_pixel=None, fn=None):
    """composite_ext_kernel<C> in float32 NumPy, operation by operation (the library is built with -ffp-contract=off).  objective: the
    pass's (kind, huber_delta, lambda_d, lambda_e).  Returns dict(image, pre, depth, weights, draw, partial, terms_partial)."""
    assert raw.dtype == F and t.dtype == F and target.dtype == F
    fn = fn or math_numpy()
    kind, hd, lam_d, lam_e = objective
    hd, lam_d, lam_e, rs = F(hd), F(lam_d), F(lam_e), F(reg_scale)
    R, S = t.shape
    C = CR.template_C(S)
    P = 64 * C
    one, zero, eps, half, two = F(1.0), F(0.0), F(1e-10), F(0.5), F(2.0)
    gs, ls = F(grad_scale), F(loss_scale)

    def lanes(a, fill):
        out = np.full((R, P), fill, F)
        out[:, :S] = a
        return out.reshape(R, 64, C)
    ok = lanes(np.ones((R, S), F), 0.0) > 0
    r, g, b, sg = (lanes(raw[..., k], 0.0) for k in range(4))
    tt = lanes(t, 0.0)
    t0 = t[:, :1].copy()
    tn = np.zeros((R, S), F)
    tn[:, :-1] = t[:, 1:]
    dl = lanes(tn - t, 0.0)
    dl.reshape(R, P)[:, S - 1:] = eps
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        ex = fn["exp"](-(sg * dl)).astype(F)
        al = np.where(ok, one - ex, zero)
        x = np.where(ok, (one - al) + eps, one)
        T = np.empty((R, 64, C), F)
        run = np.ones((R, 64), F)
        for c in range(C):
            T[:, :, c] = run
            run = run * x[:, :, c]
        inc = run
        for o in (1, 2, 4, 8, 16, 32):
            new = inc.copy()
            new[:, o:] = inc[:, o:] * inc[:, :-o]
            inc = new
        excl = np.ones((R, 64), F)
        excl[:, 1:] = inc[:, :-1]
        acc = [np.zeros((R, 64), F) for _ in range(6)]
        w = np.empty((R, 64, C), F)
        mid = np.empty((R, 64, C), F)
        for c in range(C):
            T[:, :, c] = T[:, :, c] * excl
            w[:, :, c] = al[:, :, c] * T[:, :, c]
            for k, v in enumerate((r, g, b, tt)):
                acc[k] = acc[k] + w[:, :, c] * v[:, :, c]
            acc[4] = acc[4] + w[:, :, c]
            mid[:, :, c] = (tt[:, :, c] - t0) + half * dl[:, :, c]
            acc[5] = acc[5] + w[:, :, c] * mid[:, :, c]
        lw, lm = acc[4], acc[5]
        sr, sgc, sb, sd, sw = (CR._wave_sum(v) for v in acc[:5])
        pre = np.stack([sr, sgc, sb], axis=-1)
        if white:
            pre = pre + (one - sw)[:, None]
        img = np.minimum(np.maximum(pre, zero), one)
        tgt = target.copy()
        if own_pixel is not None:
            tgt[own_pixel] = img[own_pixel]
        df = img - tgt
        ad = np.abs(df)
        if kind == MAE:
            rho, h = ad, np.where(df > 0, half, np.where(df < 0, -half, zero)).astype(F)
        elif kind == HUBER:
            rho, h = np.where(ad <= hd, half * (df * df), hd * (ad - half * hd)).astype(F), half * np.minimum(np.maximum(df, -hd), hd)
        elif kind == LOG_COSH:
            rho, h = (ad + fn["log1p"](fn["exp"](F(-2.0) * ad))) - F(0.693147180559945), half * fn["tanh"](df)
        else:
            rho, h = df * df, df
        rho, h = rho.astype(F), h.astype(F)
        l2 = ((zero + df[:, 0] * df[:, 0]) + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]
        lp = ((zero + rho[:, 0]) + rho[:, 1]) + rho[:, 2]
        gi = np.where((pre >= zero) & (pre <= one), gs * h, zero).astype(F)
        # distortion scans, entropy
        Wr, Mr = _scan_add_exclusive(lw), _scan_add_exclusive(lm)
        Mtot = CR._wave_sum(lm)[:, None]
        swl = sw[:, None]
        ac = np.minimum(np.maximum(sw, ACC_LO), ACC_HI)
        H = (-ac * fn["log"](ac)) - (one - ac) * fn["log"](one - ac)
        dH = np.where((sw >= ACC_LO) & (sw <= ACC_HI), fn["log"]((one - ac) / ac), zero).astype(F)[:, None]
        has_reg = lam_d != 0 or lam_e != 0
        gsum = ((gi[:, 0] + gi[:, 1]) + gi[:, 2]) if white else np.zeros(R, F)
        g0, g1, g2, gsum = (v[:, None] for v in (gi[:, 0], gi[:, 1], gi[:, 2], gsum))
        dw = np.empty((R, 64, C), F)
        dpart = np.zeros((R, 64), F)
        for c in range(C):
            wc, m = w[:, :, c], mid[:, :, c]
            dwc = ((g0 * r[:, :, c] + g1 * g[:, :, c]) + g2 * b[:, :, c]) - gsum
            wm = wc * m
            before = m * Wr - Mr
            Ws, Ms = (swl - Wr) - wc, (Mtot - Mr) - wm
            gD = two * ((before + Ms) - m * Ws) + F(0.666666666666667) * (wc * dl[:, :, c])
            dpart = dpart + (two * (wc * before) + F(0.333333333333333) * ((wc * wc) * dl[:, :, c]))
            if has_reg:
                dwc = dwc + rs * (lam_d * gD + lam_e * dH)
            dw[:, :, c] = dwc
            Wr, Mr = Wr + wc, Mr + wm
        tD, tH = CR._wave_sum(dpart) * rs, H * rs
        lray = lp * ls
        if has_reg:
            lray = lray + (lam_d * tD + lam_e * tH)

        def wg(v):
            sl = np.zeros(((R + 3) // 4) * 4, F)
            sl[:R] = v
            sl = sl.reshape(-1, 4)
            return ((sl[:, 0] + sl[:, 1]) + (sl[:, 2] + sl[:, 3])).astype(F)
        partial = wg(lray)
        terms_partial = np.stack([wg(lp * ls), wg(l2 * ls), wg(tD), wg(tH)])
        Ql = np.empty((R, 64, C), F)
        suffix = np.zeros((R, 64), F)
        for c in range(C - 1, -1, -1):
            Ql[:, :, c] = suffix
            suffix = suffix + dw[:, :, c] * w[:, :, c]
        incs = suffix
        for o in (1, 2, 4, 8, 16, 32):
            new = incs.copy()
            new[:, :-o] = incs[:, :-o] + incs[:, o:]
            incs = new
        excls = np.zeros((R, 64), F)
        excls[:, :-1] = incs[:, 1:]
        Q = Ql + excls[:, :, None]
        dalpha = dw * T - Q / x
        dsig = (dalpha * dl) * ex
        draw = np.stack([w * g0[:, :, None], w * g1[:, :, None], w * g2[:, :, None], dsig], axis=-1)
    flat = lambda a: a.reshape(R, P, *a.shape[3:])[:, :S]
    return dict(image=img, pre=pre, depth=sd, weights=flat(w), draw=flat(draw).astype(F), partial=partial, terms_partial=terms_partial)


# ------------------------------------------------------------------------------------------------------------ exclusions
def left_out(ref, cls, objective):
    """(rays left out of the gated comparisons, how many of them are not of class UNSORTED)"""
    _, _, lam_d, lam_e = objective
    skip = CR.undecidable(ref)
    if lam_e != 0:
        skip = skip | (np.abs(ref["acc"] - float(ACC_LO)) < ACC_EDGE) | (np.abs(ref["acc"] - float(ACC_HI)) < ACC_EDGE)
    n_other = int(skip[cls != CR.UNSORTED].sum())
    if lam_d != 0:
        skip = skip | (cls == CR.UNSORTED)
    return skip, n_other


def errors(out, ref, skip):
    """CR.errors' figures plus, where `out` has them, the four terms (signed sums: only for deterministic evaluations)"""
    e = CR.errors(out, ref, skip)
    if "terms" in out:
        for k, name in enumerate(TERMS):
            e[name] = abs(float(out["terms"][k]) - float(ref["terms"][k]))
    return e


@functools.lru_cache(maxsize=None)
def case(S: int, white: int, name: str, nets: int = 3, net: int = 0):
    """CR.case's inputs under objective OBJECTIVES[name] (or "plain"): reference, the rays left out, tolerances.  Computed once, shared."""
    c = CR.case(S, white)
    obj = PLAIN if name == "plain" else OBJECTIVES[name]
    R = len(c["cls"])
    gs, ls, rs = c["grad_scale"], c["loss_scale"], 1.0 / R
    ref = reference(c["raw"], c["t"], c["target"], white, gs, ls, rs, obj, net=net, nets=nets, own_pixel=c["own"], loss0=CR.LOSS0)
    skip, n_other = left_out(ref, c["cls"], obj)
    # what the exclusions rest on: few rays are left out, and the entropy gate is open on many
    assert n_other <= 2, (S, white, name, n_other)
    inside = int(((ref["acc"] > float(ACC_LO)) & (ref["acc"] < float(ACC_HI))).sum())
    assert inside >= 20, (S, white, name, inside)
    on = (nets >> net) & 1
    pass_obj = obj if on else (obj[0], obj[1], 0.0, 0.0)
    errs = {}
    for label, fn in (("numpy", math_numpy()), ("jitter", math_jittered(7 + S))):
        m = mirror32(c["raw"], c["t"], c["target"], white, gs, ls, rs, pass_obj, own_pixel=c["own"], fn=fn)
        e = CR.errors(m, ref, skip)
        e["loss"] = CR.loss_mirror_error(m["partial"], ref["partial"], CR.LOSS0)
        for k, tname in enumerate(TERMS):
            e[tname] = CR.loss_mirror_error(m["terms_partial"][k], ref["terms_partial"][k], 0.0)
        errs[label] = e
    mirror = {k: max(errs["numpy"][k], errs["jitter"][k]) for k in errs["numpy"]}
    tol = {k: CR.TOL_FACTOR * v for k, v in mirror.items()}
    for a in [v for v in ref.values() if isinstance(v, np.ndarray)] + [skip]:
        a.setflags(write=False)
    return dict(c, objective=obj, pass_objective=pass_obj, reg_scale=rs, ref=ref, skip=skip, mirror_err=mirror, mirror_errs=errs, tol=tol,
                inside=inside, n_left_out=n_other)
