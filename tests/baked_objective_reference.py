"""NumPy reference of the extended objective of the baked-field optimisers (include/knerf.h knerf_baked_train_rays_ext), written from
the specification, not from the kernel: the four photometric losses, the distortion and opacity-entropy regularisers of a ray's weights,
and the gradient with respect to every sigma and SH coefficient of the lattice.  Everything takes a dtype: float64 is the reference,
float32 its own rounding error (the tests' yardstick).

The march is that of tests/baked_train_reference.py (samples, cells, support, trilinear weights, compositing order, termination cut);
what is added is the index of every fetched sample on its ray, from which m_j = (i_j - i_first) delta.  D is evaluated in prefix form,
the sum over later samples is a reverse cumulative sum (NOT the kernel's total minus prefix; mirror=True evaluates the regularisers'
share in the kernel's order, for the tests' tolerance).
"""
import numpy as np

from tests import baked_reference as R

MSE, MAE, HUBER, LOG_COSH = 0, 1, 2, 3
KINDS = {"mse": MSE, "mae": MAE, "huber": HUBER, "log_cosh": LOG_COSH}
CLAMP = 1e-4                      # a = clamp(O, CLAMP, 1 - CLAMP)
TERMS = ("photometric", "mse", "distortion", "opacity_entropy")


def rho(d, kind, huber_delta, f=np.float64):
    """(rho(d), rho'(d)) elementwise for a loss kind; sign(0) = 0"""
    d = np.asarray(d, dtype=f)
    a = np.abs(d)
    if kind == MSE:
        return d * d, f(2) * d
    if kind == MAE:
        return a, np.sign(d).astype(f)
    if kind == HUBER:
        h = f(huber_delta)
        inside = a <= h
        return np.where(inside, f(0.5) * d * d, h * (a - f(0.5) * h)).astype(f), np.where(inside, d, h * np.sign(d)).astype(f)
    if kind == LOG_COSH:
        return (a + np.log1p(np.exp(f(-2) * a)) - f(np.log(2.0))).astype(f), np.tanh(d).astype(f)
    raise ValueError(f"unknown loss kind {kind!r}")


def distortion_prefix(w, m, delta, f=np.float64):
    """(D, dD/dw [M]) in prefix form: D = 2 sum_k w_k (m_k W_k - M_k) + delta / 3 sum w_k^2 with the exclusive prefixes W, M"""
    w, m = np.asarray(w, dtype=f), np.asarray(m, dtype=f)
    if not w.size:
        return f(0), np.zeros(0, dtype=f)
    W = np.concatenate([np.zeros(1, dtype=f), np.cumsum(w, dtype=f)[:-1]])
    wm = (w * m).astype(f)
    M = np.concatenate([np.zeros(1, dtype=f), np.cumsum(wm, dtype=f)[:-1]])
    O, MT = np.cumsum(w, dtype=f)[-1], np.cumsum(wm, dtype=f)[-1]
    D = f(2) * np.cumsum(w * (m * W - M), dtype=f)[-1] + f(delta) / f(3) * np.cumsum(w * w, dtype=f)[-1]
    dD = f(2) * (f(2) * m * W - f(2) * M + MT - m * O) + f(2) / f(3) * f(delta) * w
    return f(D), dD.astype(f)


def distortion_definition(w, m, delta):
    """D = sum_i sum_j w_i w_j |m_i - m_j| + delta / 3 sum_i w_i^2, the O(S^2) definition in float64"""
    w, m = np.asarray(w, dtype=np.float64), np.asarray(m, dtype=np.float64)
    return float((w[:, None] * w[None, :] * np.abs(m[:, None] - m[None, :])).sum() + float(delta) / 3.0 * (w * w).sum())


def entropy(O, f=np.float64):
    """(H, dH/dw) of a ray's opacity O: a = clamp(O), H = -a ln a - (1 - a) ln(1 - a); the derivative is 0 outside the clamp"""
    lo, hi = f(CLAMP), f(1) - f(CLAMP)
    a = min(max(f(O), lo), hi)
    H = -a * np.log(a) - (f(1) - a) * np.log(f(1) - a)
    dH = np.log((f(1) - a) / a) if lo <= f(O) <= hi else f(0)
    return f(H), f(dH)


def ray_objective(s, raw, index, delta, target, bg, eps, norm, kind=MSE, huber_delta=0.0, distortion=0.0, opacity_entropy=0.0,
                  f=np.float64, mirror=False):
    """One ray from its fetched samples in march order: s [M] the interpolated densities, raw [M,3] the colours before their clamp,
    index [M] the samples' indices on the ray, delta = step |d|, target [3], bg 0 or 1, eps the termination threshold (0: off), norm
    the N of the launch.  Returns a dict: "kept" (samples up to and including the one behind which the cut falls), "rho" (sum_c
    rho(d_c)), "sq" (sum_c d_c^2), "D", "H", "pre" [3], "out" [3], "O", "w" [kept], "T" [kept] (T_{j+1}), and the gradients of
    L = rho / (3 N) + distortion D / N + opacity_entropy H / N: "ds" [kept] (dL/ds_j) and "draw" [kept,3] (dL/draw_j).
    mirror: the regularisers' share of ds in the kernel's summation order (total_minus_prefix_mirror) instead of the reverse cumulative
    sum; the photometric share stays as it is."""
    s, raw = np.asarray(s, dtype=f), np.asarray(raw, dtype=f).reshape(-1, 3)
    index = np.asarray(index, dtype=np.int64)
    delta, bg, norm = f(delta), f(bg), f(norm)
    alpha = (1 - np.exp(-(s * delta))).astype(f)
    Tn = np.cumprod(1 - alpha, dtype=f)
    kept = Tn.size
    if eps > 0 and Tn.size:
        below = np.nonzero(Tn < f(eps))[0]
        if below.size:
            kept = int(below[0]) + 1
    raw, alpha, Tn, index = raw[:kept], alpha[:kept], Tn[:kept], index[:kept]
    Tb = np.concatenate([np.ones(1, dtype=f), Tn[:-1]]) if kept else Tn
    w = (Tb * alpha).astype(f)
    col = np.clip(raw, 0, 1)
    C = np.cumsum(w[:, None] * col, axis=0, dtype=f)[-1] if kept else np.zeros(3, dtype=f)
    O = np.cumsum(w, dtype=f)[-1] if kept else f(0)
    pre = C + bg * (1 - O)
    out = np.clip(pre, 0, 1)
    d = (out - np.asarray(target, dtype=f)).astype(f)
    r, dr_ = rho(d, kind, huber_delta, f)
    m = ((index - index[0]).astype(f) * delta) if kept else np.zeros(0, dtype=f)
    D, dD = distortion_prefix(w, m, delta, f)
    H, dH = entropy(O, f)
    res = {"kept": kept, "rho": f(r.sum(dtype=f)), "sq": f((d * d).sum(dtype=f)), "D": D, "H": H, "pre": pre, "out": out, "O": O, "w": w,
           "T": Tn, "ds": np.zeros(0, dtype=f), "draw": np.zeros((0, 3), dtype=f)}
    if not kept:
        return res
    g = (dr_ / (f(3) * norm)) * ((pre >= 0) & (pre <= 1))
    reg = (f(distortion) / norm) * dD + (f(opacity_entropy) / norm) * dH
    A = ((col - bg) * g[None, :]).sum(axis=1).astype(f)
    if not mirror:
        A = (A + reg).astype(f)
    wA = w * A
    later = np.concatenate([np.cumsum(wA[::-1], dtype=f)[::-1][1:], np.zeros(1, dtype=f)])     # sum over i > j
    res["ds"] = (delta * (Tn * A - later)).astype(f)
    if mirror:
        res["ds"] = (res["ds"] + total_minus_prefix_mirror(w, m, delta, Tn, f(distortion) / norm, (f(opacity_entropy) / norm) * dH, f)).astype(f)
    res["draw"] = (g[None, :] * w[:, None] * ((raw >= 0) & (raw <= 1))).astype(f)
    return res


def ray_geometry(resolution, lo, hi, o, d, near, far, step, support, f=np.float64):
    """The fetched samples of one ray on a lattice: (idx [M,8] flat lattice points, tau [M,8] trilinear weights, index [M] the samples'
    indices on the ray, |d|): baked_train_reference.loss_and_grad's placement with the indices kept"""
    Rr = np.array(resolution)
    lo = np.asarray(lo, dtype=np.float32).astype(f)
    hi = np.asarray(hi, dtype=np.float32).astype(f)
    cells = (Rr - 1).astype(f)
    scale = (cells.astype(np.float64) / (hi.astype(np.float64) - lo.astype(np.float64))).astype(np.float32).astype(f)
    h = f(np.float32(step))
    S = max(int(np.ceil((np.float64(far) - np.float64(near)) / np.float64(h))), 0)
    nrm = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    t = f(near) + (np.arange(S, dtype=f) + f(0.5)) * h
    p = o[None, :] + d[None, :] * t[:, None]
    u = (p - lo[None, :]) * scale[None, :]
    inside = np.all((u >= 0) & (u <= cells[None, :]), axis=1)
    index = np.nonzero(inside)[0]
    ui = u[inside]
    cell = np.minimum(np.floor(ui), cells[None, :] - 1).astype(np.int64)
    keep = support[cell[:, 0], cell[:, 1], cell[:, 2]]
    ui, cell, index = ui[keep], cell[keep], index[keep]
    fr = ui - cell.astype(f)
    tau = np.zeros((cell.shape[0], 8), dtype=f)
    idx = np.zeros((cell.shape[0], 8), dtype=np.int64)
    n_ = 0
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                tau[:, n_] = (fr[:, 0] if a else 1 - fr[:, 0]) * (fr[:, 1] if b else 1 - fr[:, 1]) * (fr[:, 2] if c else 1 - fr[:, 2])
                idx[:, n_] = ((cell[:, 0] + a) * Rr[1] + (cell[:, 1] + b)) * Rr[2] + (cell[:, 2] + c)
                n_ += 1
    return idx, tau, index, nrm


def loss_and_grad(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, support, white_background=False,
                  termination=0.0, loss_kind=MSE, huber_delta=0.0, distortion=0.0, opacity_entropy=0.0, dtype=np.float64, order=None,
                  n_norm=None, info=None, mirror=False):
    """(L, terms, g_sigma [Rx,Ry,Rz], g_coef [Rx,Ry,Rz,K,3]) of
        L = 1 / (3 N) sum_rays sum_c rho(d_c) + distortion / N sum_rays D + opacity_entropy / N sum_rays H,
    all arithmetic in `dtype`; terms = {"photometric", "mse", "distortion", "opacity_entropy"}: the four means (over rays and channels,
    resp. over rays), unweighted.  Arguments as baked_train_reference.loss_and_grad; loss_kind one of MSE, MAE, HUBER, LOG_COSH (or its
    name).  mirror: as ray_objective.  info: a dict that receives "terms" [N,4] (per ray: sum rho, sum d^2, D, H), "opacity" [N], "kept" [N] (fetched samples up
    to the cut), "gaps" [N] (bool: the kept indices are not consecutive), "pre" [N,3], "out" [N,3], "raw" [M,3], "T" [M]."""
    f = dtype
    kind = KINDS.get(loss_kind, loss_kind)
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
    bg = f(1.0 if white_background else 0.0)
    sg_flat, co_flat = sg.reshape(-1), co.reshape(-1, K, 3)
    g_sigma = np.zeros(sg_flat.shape, dtype=f)
    g_coef = np.zeros(co_flat.shape, dtype=f)
    per_ray = np.zeros((N, 4), dtype=np.float64)
    opa, kept, gaps, pre = np.zeros(N), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool), np.zeros((N, 3))
    raws, Ts = [], []
    for r in (range(N) if order is None else order):
        o, d = o_all[r], d_all[r]
        idx, tau, index, nrm = ray_geometry(sg.shape, lo, hi, o, d, near[r], far[r], step, support, f)
        unit = d / nrm if nrm > 0 else np.zeros(3, dtype=f)
        Y = R.real_sh(unit, degree, dtype=f)
        s_j = np.einsum("mn,mn->m", tau, sg_flat[idx]).astype(f)
        c_j = np.einsum("mn,mnkc->mkc", tau, co_flat[idx]).astype(f)
        raw = np.einsum("mkc,k->mc", c_j, Y).astype(f)
        delta = h * nrm
        res = ray_objective(s_j, raw, index, delta, tg[r], bg, eps, norm, kind, huber_delta, distortion, opacity_entropy, f, mirror)
        m = res["kept"]
        per_ray[r] = (res["rho"], res["sq"], res["D"], res["H"])
        opa[r], kept[r], pre[r] = res["O"], m, res["pre"]
        gaps[r] = m > 1 and bool((np.diff(index[:m]) > 1).any())
        raws.append(raw[:m]); Ts.append(res["T"])
        if not m:
            continue
        np.add.at(g_sigma, idx[:m], (tau[:m] * res["ds"][:, None]).astype(f))
        np.add.at(g_coef, idx[:m], (tau[:m, :, None, None] * (Y[None, None, :, None] * res["draw"][:, None, None, :])).astype(f))
    if info is not None:
        info.update(terms=per_ray, opacity=opa, kept=kept, gaps=gaps, pre=pre, out=np.clip(pre, 0, 1), raw=np.concatenate(raws) if raws else np.zeros((0, 3)),
                    T=np.concatenate(Ts) if Ts else np.zeros(0))
    tot = per_ray.sum(axis=0)
    n = float(norm)
    terms = {"photometric": tot[0] / (3.0 * n), "mse": tot[1] / (3.0 * n), "distortion": tot[2] / n, "opacity_entropy": tot[3] / n}
    L = terms["photometric"] + float(distortion) * terms["distortion"] + float(opacity_entropy) * terms["opacity_entropy"]
    return L, terms, g_sigma.reshape(sg.shape), g_coef.reshape(co.shape)


def total_minus_prefix_mirror(w, m, delta, T, wd, re, f=np.float32):
    """The kernel's summation order for the regularisers' share of dL/dsigma, in dtype f on the CPU: r_j from running prefixes,
    later_j = total - running sum_{i<=j} w_i r_i with total = wd 2 D + re O; returns delta (T_{j+1} r_j - later_j) [M].  The tests derive
    the tolerance factor of the distortion cases from its deviation from the reverse cumulative sum in float64."""
    w, m, T = (np.asarray(x, dtype=f) for x in (w, m, T))
    delta, wd, re = f(delta), f(wd), f(re)
    W = M = S1 = S2 = f(0)
    for k in range(w.size):
        S1 = f(S1 + w[k] * f(m[k] * W - M)); S2 = f(S2 + w[k] * w[k]); M = f(M + w[k] * m[k]); W = f(W + w[k])
    D, O, MT = f(f(2) * S1 + f(delta * f(f(1) / f(3))) * S2), W, M
    total = f(wd * f(f(2) * D) + re * O)
    out = np.zeros(w.size, dtype=f)
    W = M = run = f(0)
    for k in range(w.size):
        r = f(wd * f(f(2) * f(f(2) * m[k] * W - f(2) * M + MT - m[k] * O) + f(f(2) / f(3)) * delta * w[k]) + re)
        run = f(run + w[k] * r)
        M = f(M + w[k] * m[k]); W = f(W + w[k])
        out[k] = f(delta * f(T[k] * r - f(total - run)))
    return out


def optimise(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, lr_sigma, lr_sh, steps, dilation=0,
             white_background=False, termination=0.0, **objective):
    """baked_train_reference.optimise under the extended objective (loss_kind, huber_delta, distortion, opacity_entropy): the list of
    `steps` + 1 objective values, float64 on full batches with the reference adam_step"""
    from tests import baked_train_reference as T
    sg = np.asarray(sigma, dtype=np.float32)
    co = np.asarray(coefficients, dtype=np.float16)
    K = co.shape[3]
    support = T.support_cells(sg, dilation)
    slots = T.slot_points(support).reshape(-1)
    train = T.sigma_trainable(support).reshape(-1)[slots]
    w = np.concatenate([sg.reshape(-1, 1)[slots].astype(np.float64) * train[:, None], co.reshape(-1, 3 * K)[slots].astype(np.float64)], axis=1)
    m, v = np.zeros_like(w), np.zeros_like(w)
    args = (lo, hi, origins, directions, near, far, step, target, support, white_background, termination)
    values = []
    for t in range(1, steps + 1):
        L, _, gs, gc = loss_and_grad(sg, co.astype(np.float64), *args, **objective)
        values.append(L)
        g = np.concatenate([gs.reshape(-1, 1)[slots], gc.reshape(-1, 3 * K)[slots]], axis=1)
        w, m, v, s32, c16 = T.adam_step(w, m, v, g, train, lr_sigma, lr_sh, 0.9, 0.999, 1e-7, t)
        sg = sg.copy().reshape(-1); sg[slots] = s32; sg = sg.reshape(sigma.shape)
        cf = co.copy().reshape(-1, 3 * K); cf[slots] = c16; co = cf.reshape(co.shape)
    values.append(loss_and_grad(sg, co.astype(np.float64), *args, **objective)[0])
    return values
