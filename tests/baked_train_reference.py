"""NumPy reference of optimising a baked field (include/knerf.h knerf_baked_train_rays / knerf_baked_train_apply), written from the
specification, not from the kernels: the squared-error loss of the baked march and its gradient with respect to every sigma and SH
coefficient of the lattice, the support / slot / trainable-sigma construction, and the Adam + projection + fp16 repack step.
Everything takes a dtype: float64 is the reference, float32 its own rounding error (the tests' yardstick).

The march is that of tests/baked_reference.py march (samples, cells, trilinear weights, compositing order); here the samples of a ray
are restricted to the cells of a SUPPORT and the sums a gradient needs are kept.
"""
import numpy as np

from tests import baked_reference as R


# ---- support, slots, trainable sigma
def support_cells(sigma, dilation=0):
    """bool [Rx-1,Ry-1,Rz-1]: the occupied cells (a corner has sigma > 0) grown by `dilation` cells in Chebyshev distance"""
    occ = R.occupied_cells(sigma)
    d = int(dilation)
    if d == 0:
        return occ
    pad = np.pad(occ, d, constant_values=False)
    out = np.zeros_like(occ)
    cx, cy, cz = occ.shape
    for a in range(2 * d + 1):
        for b in range(2 * d + 1):
            for c in range(2 * d + 1):
                out |= pad[a:a + cx, b:b + cy, c:c + cz]
    return out


def slot_points(support):
    """bool [Rx,Ry,Rz]: the lattice points that are a corner of a support cell"""
    return R.touched_points(support)


def sigma_trainable(support):
    """bool [Rx,Ry,Rz]: slots whose 8 adjacent cells ALL lie in the support or outside the lattice"""
    pad = np.pad(support, 1, constant_values=True)
    ok = np.ones(tuple(c + 1 for c in support.shape), dtype=bool)
    rx, ry, rz = ok.shape
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                ok &= pad[a:a + rx, b:b + ry, c:c + rz]
    return ok & slot_points(support)


# ---- loss and gradient
def loss_and_grad(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, support, white_background=False,
                  termination=0.0, dtype=np.float64, order=None, n_norm=None, info=None):
    """(L, g_sigma [Rx,Ry,Rz], g_coef [Rx,Ry,Rz,K,3], out [N,3]) of L = (1 / 3 N) sum_rays sum_c (out_c - target_c)^2, all arithmetic
    in `dtype`.  sigma, coefficients (already rounded to fp16), lo / hi, near / far, step: as baked_reference.march.  support: bool
    cells; only samples in support cells are fetched.  order: the order in which the rays' contributions are accumulated (default
    0..N-1).  n_norm: the N of the normalisation (default: the ray count).  info: a dict that receives "raw" [M,3] (the colour of every
    fetched sample before its clamp), "pre" [N,3] (every ray's output before its clamp), "opacity" [N] and "T" [M] (the transmittance
    behind every fetched sample)."""
    f = dtype
    sg = np.asarray(sigma, dtype=f)
    co = np.asarray(coefficients, dtype=f)
    Rr = np.array(sg.shape)
    K = co.shape[3]
    degree = int(round(np.sqrt(K))) - 1
    lo = np.asarray(lo, dtype=np.float32).astype(f)
    hi = np.asarray(hi, dtype=np.float32).astype(f)
    cells = (Rr - 1).astype(f)
    scale = (cells.astype(np.float64) / (hi.astype(np.float64) - lo.astype(np.float64))).astype(np.float32).astype(f)
    o_all = np.asarray(origins, dtype=np.float32).astype(f)
    d_all = np.asarray(directions, dtype=np.float32).astype(f)
    tg = np.asarray(target, dtype=np.float32).astype(f)
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
    out_all, pre_all, opa_all = np.zeros((N, 3), dtype=f), np.zeros((N, 3), dtype=f), np.zeros(N, dtype=f)
    raws, Ts = [], []
    sq_total = 0.0
    for r in (range(N) if order is None else order):
        o, d = o_all[r], d_all[r]
        S = max(int(np.ceil((np.float64(far[r]) - np.float64(near[r])) / np.float64(h))), 0)
        nrm = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        unit = d / nrm if nrm > 0 else np.zeros(3, dtype=f)
        Y = R.real_sh(unit, degree, dtype=f)
        t = near[r] + (np.arange(S, dtype=f) + f(0.5)) * h
        p = o[None, :] + d[None, :] * t[:, None]
        u = (p - lo[None, :]) * scale[None, :]
        inside = np.all((u >= 0) & (u <= cells[None, :]), axis=1)
        ui = u[inside]
        cell = np.minimum(np.floor(ui), cells[None, :] - 1).astype(np.int64)
        keep = support[cell[:, 0], cell[:, 1], cell[:, 2]]
        ui, cell = ui[keep], cell[keep]
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
        s_j = np.einsum("mn,mn->m", tau, sg_flat[idx]).astype(f)
        c_j = np.einsum("mn,mnkc->mkc", tau, co_flat[idx]).astype(f)
        raw = np.einsum("mkc,k->mc", c_j, Y).astype(f)
        delta = h * nrm
        alpha = (1 - np.exp(-(s_j * delta))).astype(f)
        Tn = np.cumprod(1 - alpha, dtype=f)                                 # T_{j+1}, in ascending sample order
        if eps > 0 and Tn.size:
            below = np.nonzero(Tn < eps)[0]
            if below.size:                                                  # the first sample behind which T < eps is the last one
                m = below[0] + 1
                tau, idx, raw, alpha, Tn = tau[:m], idx[:m], raw[:m], alpha[:m], Tn[:m]
        Tb = np.concatenate([np.ones(1, dtype=f), Tn[:-1]]) if Tn.size else Tn
        w = (Tb * alpha).astype(f)
        col = np.clip(raw, 0, 1)
        C = np.cumsum(w[:, None] * col, axis=0, dtype=f)[-1] if w.size else np.zeros(3, dtype=f)
        O = np.cumsum(w, dtype=f)[-1] if w.size else f(0)
        pre = C + bg * (1 - O)
        out = np.clip(pre, 0, 1)
        out_all[r], pre_all[r], opa_all[r] = out, pre, O
        diff = out - tg[r]
        sq_total += float(np.sum(diff.astype(np.float64) ** 2)) if f is np.float64 else float(np.sum(diff * diff, dtype=f))
        raws.append(raw); Ts.append(Tn)
        if not w.size:
            continue
        g = (f(2) * diff / (f(3) * norm)) * ((pre >= 0) & (pre <= 1))
        dr = g[None, :] * w[:, None] * ((raw >= 0) & (raw <= 1))
        A = ((col - bg) * g[None, :]).sum(axis=1).astype(f)
        wA = w * A
        later = np.concatenate([np.cumsum(wA[::-1], dtype=f)[::-1][1:], np.zeros(1, dtype=f)])     # sum over i > j
        ds = delta * (Tn * A - later)
        np.add.at(g_sigma, idx, (tau * ds[:, None]).astype(f))
        np.add.at(g_coef, idx, (tau[:, :, None, None] * (Y[None, None, :, None] * dr[:, None, None, :])).astype(f))
    if info is not None:
        info["raw"] = np.concatenate(raws) if raws else np.zeros((0, 3))
        info["T"] = np.concatenate(Ts) if Ts else np.zeros(0)
        info["pre"], info["opacity"] = pre_all, opa_all
    L = sq_total / (3.0 * float(norm))
    return L, g_sigma.reshape(sg.shape), g_coef.reshape(co.shape), out_all


# ---- Adam, projection, repack
def adam_step(master, m, v, grad, trainable, lr_sigma, lr_sh, beta_1, beta_2, epsilon, t, dtype=np.float64):
    """One Keras-form Adam step (tests/adam_reference.py adam_fp64's form: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), epsilon outside the
    root) on rows [n, 1 + 3 K] (sigma first), t the step applied (from 1).  Column 0 uses lr_sigma, is updated only where `trainable`
    [n] is set (elsewhere value and moments stay) and is projected to >= 0.  Returns (master, m, v, sigma fp32 [n], coefficients fp16
    [n, 3 K]): the new rows and what the records hold.  dtype float32: lr_t in double rounded once, one rounding per operation, the
    moments in the kernel's form m += (g - m)(1 - b1)."""
    f = dtype
    w, m, v, g = (np.array(x, dtype=f) for x in (master, m, v, grad))
    tr = np.asarray(trainable, dtype=bool)
    rate = np.empty(w.shape[1], dtype=np.float64)
    corr = np.sqrt(1.0 - float(beta_2) ** t) / (1.0 - float(beta_1) ** t)
    rate[0], rate[1:] = lr_sigma * corr, lr_sh * corr
    rate = rate.astype(f)
    upd = np.ones(w.shape, dtype=bool)
    upd[:, 0] = tr
    if f is np.float64:
        m2 = beta_1 * m + (1 - beta_1) * g
        v2 = beta_2 * v + (1 - beta_2) * g * g
    else:
        m2 = m + (g - m) * (f(1) - f(beta_1))
        v2 = v + (g * g - v) * (f(1) - f(beta_2))
    w2 = w - rate[None, :] * m2 / (np.sqrt(v2) + f(epsilon))
    m, v, w = np.where(upd, m2, m), np.where(upd, v2, v), np.where(upd, w2, w)
    w[:, 0] = np.maximum(w[:, 0], 0)
    return w, m, v, w[:, 0].astype(np.float32), w[:, 1:].astype(np.float16)


def optimise(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, lr_sigma, lr_sh, steps, dilation=0,
             beta_1=0.9, beta_2=0.999, epsilon=1e-7, white_background=False, termination=0.0):
    """The optimiser in float64 on full batches: the list of `steps` + 1 losses (before every step and after the last).  Like the
    product, the march sees sigma as fp32 and the coefficients as fp16 values while the master copy keeps every digit."""
    sg = np.asarray(sigma, dtype=np.float32)
    co = np.asarray(coefficients, dtype=np.float16)
    K = co.shape[3]
    support = support_cells(sg, dilation)
    slots = slot_points(support).reshape(-1)
    train = sigma_trainable(support).reshape(-1)[slots]
    w = np.concatenate([sg.reshape(-1, 1)[slots].astype(np.float64) * train[:, None], co.reshape(-1, 3 * K)[slots].astype(np.float64)], axis=1)
    m, v = np.zeros_like(w), np.zeros_like(w)
    args = (lo, hi, origins, directions, near, far, step, target, support, white_background, termination)
    losses = []
    for t in range(1, steps + 1):
        L, gs, gc, _ = loss_and_grad(sg, co.astype(np.float64), *args)
        losses.append(L)
        g = np.concatenate([gs.reshape(-1, 1)[slots], gc.reshape(-1, 3 * K)[slots]], axis=1)
        w, m, v, s32, c16 = adam_step(w, m, v, g, train, lr_sigma, lr_sh, beta_1, beta_2, epsilon, t)
        sg = sg.copy().reshape(-1); sg[slots] = s32; sg = sg.reshape(sigma.shape)
        cf = co.copy().reshape(-1, 3 * K); cf[slots] = c16; co = cf.reshape(co.shape)
    losses.append(loss_and_grad(sg, co.astype(np.float64), *args)[0])
    return losses
