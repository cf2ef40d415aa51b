"""NumPy reference of the rgba objective of the baked-field optimisers (include/knerf.h knerf_baked_train_rays_rgba), written from the
specification, not from the kernel: a background per ray, the target recomposited over it with the photograph's alpha, and the opacity
loss (O - alpha)^2 beside the losses and regularisers of tests/baked_objective_reference.py, on which it builds (march, rho, D, H).
Everything takes a dtype: float64 is the reference, float32 its own rounding error (the tests' yardstick); mirror=True evaluates the
regularisers' share (the opacity term included) in the kernel's summation order, total minus running prefix.
"""
import numpy as np

from tests import baked_objective_reference as Q
from tests import baked_reference as R

TERMS = Q.TERMS + ("opacity",)


def recompose(target, alpha, background, stored, f=np.float64):
    """target + (1 - alpha)(background - stored): a target stored as alpha rgb + (1 - alpha) stored, over `background`; not clipped"""
    target, background = np.asarray(target, dtype=f), np.asarray(background, dtype=f)
    return (target + ((f(1) - np.asarray(alpha, dtype=f))[..., None] * (background - f(stored)))).astype(f)


def ray_objective(s, raw, index, delta, target, b, alpha, stored, eps, norm, kind=Q.MSE, huber_delta=0.0, distortion=0.0,
                  opacity_entropy=0.0, opacity=0.0, f=np.float64, mirror=False):
    """Q.ray_objective with b [3] the ray's background, alpha its photograph's alpha (None: the target is used as it is and alpha reads
    as 1), stored 0 or 1 and opacity the weight lambda_o.  The dict also holds "op" = (O - alpha)^2 and "tgt" [3]."""
    s, raw = np.asarray(s, dtype=f), np.asarray(raw, dtype=f).reshape(-1, 3)
    index = np.asarray(index, dtype=np.int64)
    delta, norm, b = f(delta), f(norm), np.asarray(b, dtype=f)
    al = f(1) if alpha is None else f(alpha)
    a = (1 - np.exp(-(s * delta))).astype(f)
    Tn = np.cumprod(1 - a, dtype=f)
    kept = Tn.size
    if eps > 0 and Tn.size:
        below = np.nonzero(Tn < f(eps))[0]
        if below.size:
            kept = int(below[0]) + 1
    raw, a, Tn, index = raw[:kept], a[:kept], Tn[:kept], index[:kept]
    Tb = np.concatenate([np.ones(1, dtype=f), Tn[:-1]]) if kept else Tn
    w = (Tb * a).astype(f)
    col = np.clip(raw, 0, 1)
    C = np.cumsum(w[:, None] * col, axis=0, dtype=f)[-1] if kept else np.zeros(3, dtype=f)
    O = np.cumsum(w, dtype=f)[-1] if kept else f(0)
    pre = (C + b * (f(1) - O)).astype(f)
    out = np.clip(pre, 0, 1)
    tg = np.asarray(target, dtype=f)
    tgt = tg if alpha is None else (tg + (f(1) - al) * (b - f(stored))).astype(f)
    d = (out - tgt).astype(f)
    r, dr_ = Q.rho(d, kind, huber_delta, f)
    m = ((index - index[0]).astype(f) * delta) if kept else np.zeros(0, dtype=f)
    D, dD = Q.distortion_prefix(w, m, delta, f)
    H, dH = Q.entropy(O, f)
    res = {"kept": kept, "rho": f(r.sum(dtype=f)), "sq": f((d * d).sum(dtype=f)), "D": D, "H": H, "op": f((O - al) * (O - al)), "pre": pre,
           "out": out, "tgt": tgt, "O": O, "w": w, "T": Tn, "ds": np.zeros(0, dtype=f), "draw": np.zeros((0, 3), dtype=f)}
    if not kept:
        return res
    g = (dr_ / (f(3) * norm)) * ((pre >= 0) & (pre <= 1))
    re = (f(opacity_entropy) / norm) * dH
    if opacity > 0:
        re = f(re + (f(opacity) / norm) * (f(2) * (O - al)))
    reg = (f(distortion) / norm) * dD + re
    A = ((col - b[None, :]) * g[None, :]).sum(axis=1).astype(f)
    if not mirror:
        A = (A + reg).astype(f)
    wA = w * A
    later = np.concatenate([np.cumsum(wA[::-1], dtype=f)[::-1][1:], np.zeros(1, dtype=f)])     # sum over i > j
    res["ds"] = (delta * (Tn * A - later)).astype(f)
    if mirror:
        res["ds"] = (res["ds"] + Q.total_minus_prefix_mirror(w, m, delta, Tn, f(distortion) / norm, re, f)).astype(f)
    res["draw"] = (g[None, :] * w[:, None] * ((raw >= 0) & (raw <= 1))).astype(f)
    return res


def loss_and_grad(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, support, background=None, alpha=None,
                  stored=0.0, white_background=False, termination=0.0, loss_kind=Q.MSE, huber_delta=0.0, distortion=0.0,
                  opacity_entropy=0.0, opacity=0.0, dtype=np.float64, order=None, n_norm=None, info=None, mirror=False):
    """(L, terms, g_sigma [Rx,Ry,Rz], g_coef [Rx,Ry,Rz,K,3]) of
        L = 1 / (3 N) sum rho(d_c) + distortion / N sum D + opacity_entropy / N sum H + opacity / N sum (O - alpha)^2
    with d = clip(C + b (1 - O), 0, 1) - (target + (1 - alpha)(b - stored)); background [N,3] or None (the flag's colour on every
    channel), alpha [N] or None.  The other arguments, `info` and `mirror` as Q.loss_and_grad; terms has the five means of TERMS and
    info also "tgt" [N,3]."""
    f = dtype
    kind = Q.KINDS.get(loss_kind, loss_kind)
    sg = np.asarray(sigma, dtype=f)
    co = np.asarray(coefficients, dtype=f)
    K = co.shape[3]
    degree = int(round(np.sqrt(K))) - 1
    o_all = np.asarray(origins, dtype=np.float32).astype(f)
    d_all = np.asarray(directions, dtype=np.float32).astype(f)
    tg = np.asarray(target)
    tg = tg.astype(f) if tg.dtype == np.float64 else tg.astype(np.float32).astype(f)       # float64 targets are taken as they are
    N = o_all.shape[0]
    norm = f(N if n_norm is None else n_norm)
    near = np.broadcast_to(np.asarray(near, dtype=np.float32), (N,)).astype(f)
    far = np.broadcast_to(np.asarray(far, dtype=np.float32), (N,)).astype(f)
    h = f(np.float32(step))
    eps = f(np.float32(termination))
    if background is None:
        bg = np.full((N, 3), 1.0 if white_background else 0.0, dtype=f)
    else:
        bg = np.asarray(background, dtype=np.float32).astype(f)
    al = None if alpha is None else np.asarray(alpha, dtype=np.float32).astype(f)
    sg_flat, co_flat = sg.reshape(-1), co.reshape(-1, K, 3)
    g_sigma = np.zeros(sg_flat.shape, dtype=f)
    g_coef = np.zeros(co_flat.shape, dtype=f)
    per_ray = np.zeros((N, 5), dtype=np.float64)
    opa, kept, gaps = np.zeros(N), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool)
    pre, tgt = np.zeros((N, 3)), np.zeros((N, 3))
    raws, Ts = [], []
    for r in (range(N) if order is None else order):
        o, d = o_all[r], d_all[r]
        idx, tau, index, nrm = Q.ray_geometry(sg.shape, lo, hi, o, d, near[r], far[r], step, support, f)
        unit = d / nrm if nrm > 0 else np.zeros(3, dtype=f)
        Y = R.real_sh(unit, degree, dtype=f)
        s_j = np.einsum("mn,mn->m", tau, sg_flat[idx]).astype(f)
        c_j = np.einsum("mn,mnkc->mkc", tau, co_flat[idx]).astype(f)
        raw = np.einsum("mkc,k->mc", c_j, Y).astype(f)
        delta = h * nrm
        res = ray_objective(s_j, raw, index, delta, tg[r], bg[r], None if al is None else al[r], stored, eps, norm, kind, huber_delta,
                            distortion, opacity_entropy, opacity, f, mirror)
        m = res["kept"]
        per_ray[r] = (res["rho"], res["sq"], res["D"], res["H"], res["op"])
        opa[r], kept[r], pre[r], tgt[r] = res["O"], m, res["pre"], res["tgt"]
        gaps[r] = m > 1 and bool((np.diff(index[:m]) > 1).any())
        raws.append(raw[:m]); Ts.append(res["T"])
        if not m:
            continue
        np.add.at(g_sigma, idx[:m], (tau[:m] * res["ds"][:, None]).astype(f))
        np.add.at(g_coef, idx[:m], (tau[:m, :, None, None] * (Y[None, None, :, None] * res["draw"][:, None, None, :])).astype(f))
    if info is not None:
        info.update(terms=per_ray, opacity=opa, kept=kept, gaps=gaps, pre=pre, out=np.clip(pre, 0, 1), tgt=tgt,
                    raw=np.concatenate(raws) if raws else np.zeros((0, 3)), T=np.concatenate(Ts) if Ts else np.zeros(0))
    tot = per_ray.sum(axis=0)
    n = float(norm)
    terms = {"photometric": tot[0] / (3.0 * n), "mse": tot[1] / (3.0 * n), "distortion": tot[2] / n, "opacity_entropy": tot[3] / n,
             "opacity": tot[4] / n}
    L = terms["photometric"] + float(distortion) * terms["distortion"] + float(opacity_entropy) * terms["opacity_entropy"] + \
        float(opacity) * terms["opacity"]
    return L, terms, g_sigma.reshape(sg.shape), g_coef.reshape(co.shape)


def optimise(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, alpha, backgrounds, lr_sigma, lr_sh, dilation=0,
             termination=0.0, stored=0.0, **objective):
    """Q.optimise under the rgba objective: one step per entry of `backgrounds` ([N,3] each, the tensors an optimiser drew) and a final
    evaluation under the first of them; the list of objective values, float64 with the reference adam_step"""
    from tests import baked_train_reference as T
    sg = np.asarray(sigma, dtype=np.float32)
    co = np.asarray(coefficients, dtype=np.float16)
    K = co.shape[3]
    support = T.support_cells(sg, dilation)
    slots = T.slot_points(support).reshape(-1)
    train = T.sigma_trainable(support).reshape(-1)[slots]
    w = np.concatenate([sg.reshape(-1, 1)[slots].astype(np.float64) * train[:, None], co.reshape(-1, 3 * K)[slots].astype(np.float64)], axis=1)
    m, v = np.zeros_like(w), np.zeros_like(w)
    geo = (lo, hi, origins, directions, near, far, step, target, support)
    values = []
    for t, bg in enumerate(list(backgrounds) + [backgrounds[0]], start=1):
        L, _, gs, gc = loss_and_grad(sg, co.astype(np.float64), *geo, background=bg, alpha=alpha, stored=stored, termination=termination,
                                     **objective)
        values.append(L)
        if t > len(backgrounds):
            break
        g = np.concatenate([gs.reshape(-1, 1)[slots], gc.reshape(-1, 3 * K)[slots]], axis=1)
        w, m, v, s32, c16 = T.adam_step(w, m, v, g, train, lr_sigma, lr_sh, 0.9, 0.999, 1e-7, t)
        sg = sg.copy().reshape(-1); sg[slots] = s32; sg = sg.reshape(sigma.shape)
        cf = co.copy().reshape(-1, 3 * K); cf[slots] = c16; co = cf.reshape(co.shape)
    return values
