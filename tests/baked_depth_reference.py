"""NumPy reference of the depth-supervised objective of the baked-field optimisers (include/knerf.h knerf_baked_train_rays_depth), written
from the specification, not from the kernel: the rgba objective of tests/baked_rgba_reference.py, on which it builds (march, rho, D, H,
backgrounds, alphas), plus the depth term c (Z - z*)^2 between a ray's expected depth Z = sum w_j t_j and a target z* of weight c.
Everything takes a dtype: float64 is the reference, float32 its own rounding error (the tests' yardstick); mirror=True evaluates the
share of every term of the weights (the depth term included) in the kernel's summation order, total minus running prefix.

The depth term is linear in the weights through Z:  dL/dw_j = zeta t_j,  zeta = (depth / N) 2 c (Z - z*),  sum_j w_j dL/dw_j = zeta Z.
A ray of weight 0 has term and zeta exactly 0 whatever its z* (NaN included).
"""
import numpy as np

from tests import baked_objective_reference as Q
from tests import baked_reference as R
from tests import baked_rgba_reference as P

TERMS = P.TERMS + ("depth",)


def depth_share(w, t, Tn, delta, zeta, f=np.float64, mirror=False):
    """the depth term's share of dL/ds_j [M]: delta (T_{j+1} zeta t_j - sum_{i>j} w_i zeta t_i); the sum over later samples is a reverse
    cumulative sum, or with mirror the kernel's total (zeta Z, Z summed in march order) minus a running prefix, in dtype f"""
    w, t, Tn = (np.asarray(x, dtype=f) for x in (w, t, Tn))
    delta, zeta = f(delta), f(zeta)
    r = (zeta * t).astype(f)
    if not mirror:
        wr = (w * r).astype(f)
        later = np.concatenate([np.cumsum(wr[::-1], dtype=f)[::-1][1:], np.zeros(1, dtype=f)])
        return (delta * (Tn * r - later)).astype(f)
    Z = f(0)
    for k in range(w.size):
        Z = f(Z + w[k] * t[k])
    total, run = f(zeta * Z), f(0)
    out = np.zeros(w.size, dtype=f)
    for k in range(w.size):
        run = f(run + w[k] * r[k])
        out[k] = f(delta * f(Tn[k] * r[k] - f(total - run)))
    return out


def loss_and_grad(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, support, background=None, alpha=None,
                  stored=0.0, white_background=False, termination=0.0, loss_kind=Q.MSE, huber_delta=0.0, distortion=0.0,
                  opacity_entropy=0.0, opacity=0.0, depth_target=None, depth_weight=None, depth=0.0, dtype=np.float64, order=None,
                  n_norm=None, info=None, mirror=False):
    """(L, terms, g_sigma [Rx,Ry,Rz], g_coef [Rx,Ry,Rz,K,3]) of
        L = P's L + depth / N sum_rays c (Z - z*)^2,   Z = sum_j w_j t_j,  t_j = near + (i_j + 0.5) step
    over the fetched samples up to the termination cut; depth_target [N] (z*), depth_weight [N] or None (c = 1).  The other arguments,
    `info` and `mirror` as P.loss_and_grad; terms has the six means of TERMS and info also "Z" [N] and "zterm" [N]."""
    f = dtype
    kind = Q.KINDS.get(loss_kind, loss_kind)
    sg = np.asarray(sigma, dtype=f)
    co = np.asarray(coefficients, dtype=f)
    K = co.shape[3]
    degree = int(round(np.sqrt(K))) - 1
    o_all = np.asarray(origins, dtype=np.float32).astype(f)
    d_all = np.asarray(directions, dtype=np.float32).astype(f)
    tg = np.asarray(target)
    tg = tg.astype(f) if tg.dtype == np.float64 else tg.astype(np.float32).astype(f)
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
    zs = np.zeros(N, dtype=f) if depth_target is None else np.asarray(depth_target, dtype=np.float32).astype(f)
    cw = np.ones(N, dtype=f) if depth_weight is None else np.asarray(depth_weight, dtype=np.float32).astype(f)
    lam = f(np.float32(depth))
    sg_flat, co_flat = sg.reshape(-1), co.reshape(-1, K, 3)
    g_sigma = np.zeros(sg_flat.shape, dtype=f)
    g_coef = np.zeros(co_flat.shape, dtype=f)
    per_ray = np.zeros((N, 6), dtype=np.float64)
    opa, kept, gaps = np.zeros(N), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool)
    pre, tgt, Zs = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N)
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
        res = P.ray_objective(s_j, raw, index, delta, tg[r], bg[r], None if al is None else al[r], stored, eps, norm, kind, huber_delta,
                              distortion, opacity_entropy, opacity, f, mirror)
        m = res["kept"]
        t = (near[r] + (index[:m].astype(f) + f(0.5)) * h).astype(f)
        w = res["w"]
        Z = f(0)
        for k in range(m):                                                 # march order, as the render kernel sums its depth
            Z = f(Z + w[k] * t[k])
        if cw[r] == 0:                                                     # a select: z* may hold anything
            zterm, zeta = f(0), f(0)
        else:
            dz = f(Z - zs[r])
            zterm, zeta = f(cw[r] * (dz * dz)), f((lam / norm) * (f(2) * (cw[r] * dz)))
        per_ray[r] = (res["rho"], res["sq"], res["D"], res["H"], res["op"], zterm)
        opa[r], kept[r], pre[r], tgt[r], Zs[r] = res["O"], m, res["pre"], res["tgt"], Z
        gaps[r] = m > 1 and bool((np.diff(index[:m]) > 1).any())
        raws.append(raw[:m]); Ts.append(res["T"])
        if not m:
            continue
        ds = res["ds"]
        if zeta != 0:
            ds = (ds + depth_share(w, t, res["T"], delta, zeta, f, mirror)).astype(f)
        np.add.at(g_sigma, idx[:m], (tau[:m] * ds[:, None]).astype(f))
        np.add.at(g_coef, idx[:m], (tau[:m, :, None, None] * (Y[None, None, :, None] * res["draw"][:, None, None, :])).astype(f))
    if info is not None:
        info.update(terms=per_ray, opacity=opa, kept=kept, gaps=gaps, pre=pre, out=np.clip(pre, 0, 1), tgt=tgt, Z=Zs, zterm=per_ray[:, 5],
                    raw=np.concatenate(raws) if raws else np.zeros((0, 3)), T=np.concatenate(Ts) if Ts else np.zeros(0))
    tot = per_ray.sum(axis=0)
    n = float(norm)
    terms = {"photometric": tot[0] / (3.0 * n), "mse": tot[1] / (3.0 * n), "distortion": tot[2] / n, "opacity_entropy": tot[3] / n,
             "opacity": tot[4] / n, "depth": tot[5] / n}
    L = terms["photometric"] + float(distortion) * terms["distortion"] + float(opacity_entropy) * terms["opacity_entropy"] + \
        float(opacity) * terms["opacity"] + float(lam) * terms["depth"]
    return L, terms, g_sigma.reshape(sg.shape), g_coef.reshape(co.shape)


def optimise(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, lr_sigma, lr_sh, steps, dilation=0,
             **objective):
    """Q.optimise under the depth-supervised objective (every keyword of loss_and_grad: background, alpha, depth_target, depth_weight,
    depth, ...): the list of `steps` + 1 objective values, float64 on full batches with the reference adam_step"""
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
    for t in range(1, steps + 1):
        L, _, gs, gc = loss_and_grad(sg, co.astype(np.float64), *geo, **objective)
        values.append(L)
        g = np.concatenate([gs.reshape(-1, 1)[slots], gc.reshape(-1, 3 * K)[slots]], axis=1)
        w, m, v, s32, c16 = T.adam_step(w, m, v, g, train, lr_sigma, lr_sh, 0.9, 0.999, 1e-7, t)
        sg = sg.copy().reshape(-1); sg[slots] = s32; sg = sg.reshape(sigma.shape)
        cf = co.copy().reshape(-1, 3 * K); cf[slots] = c16; co = cf.reshape(co.shape)
    values.append(loss_and_grad(sg, co.astype(np.float64), *geo, **objective)[0])
    return values
