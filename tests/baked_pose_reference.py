"""NumPy reference of refining camera poses against a baked field (include/knerf.h knerf_baked_ray_gradients / knerf_pose_gradients,
keras_nerf_amd/baked_pose.py PoseOptimizer), written from the specification, not from the kernels: the gradient of the squared-error
loss of the baked march with respect to every ray's origin and direction, its reduction to one rigid-motion gradient per camera, and
the Adam + Rodrigues pose update.  Everything takes a dtype: float64 is the reference, float32 its own rounding error (the tests'
yardstick).  For a brick field the reference is this one applied to the arrays of to_dense().

The march, the loss and dL/dsigma_j, dL/dr_jc are those of tests/baked_train_reference.py loss_and_grad (whose loss is also what the
central differences of tests/test_baked_pose_host.py difference); here they stay on the ray instead of going to the lattice.
"""
import numpy as np

from tests import baked_reference as R


def real_sh_grad(v, degree, dtype=np.float64):
    """[K, 3]: the gradient (d/dx, d/dy, d/dz) of the polynomials of baked_reference.real_sh as they are written, at one vector v [3]"""
    f = dtype
    x, y, z = (f(c) for c in np.asarray(v, dtype=dtype))
    pi = np.pi
    D = np.zeros((R.n_coeff(degree), 3), dtype=dtype)
    if degree >= 1:
        c = f(np.sqrt(3.0 / (4.0 * pi)))
        D[1, 1], D[2, 2], D[3, 0] = c, c, c
    if degree >= 2:
        a, b = f(0.5 * np.sqrt(15.0 / pi)), f(0.25 * np.sqrt(5.0 / pi))
        D[4] = (a * y, a * x, 0)
        D[5] = (0, a * z, a * y)
        D[6] = (0, 0, f(6.0) * b * z)
        D[7] = (a * z, 0, a * x)
        D[8] = (a * x, -a * y, 0)                       # (a / 2) (x^2 - y^2)
    if degree >= 3:
        a, b = f(0.25 * np.sqrt(35.0 / (2.0 * pi))), f(0.5 * np.sqrt(105.0 / pi))
        c, d = f(0.25 * np.sqrt(21.0 / (2.0 * pi))), f(0.25 * np.sqrt(7.0 / pi))
        xx, yy, zz = x * x, y * y, z * z
        D[9] = (f(6.0) * a * x * y, f(3.0) * a * (xx - yy), 0)
        D[10] = (b * y * z, b * x * z, b * x * y)
        D[11] = (0, c * (f(5.0) * zz - f(1.0)), f(10.0) * c * y * z)
        D[12] = (0, 0, d * (f(15.0) * zz - f(3.0)))
        D[13] = (c * (f(5.0) * zz - f(1.0)), 0, f(10.0) * c * x * z)
        D[14] = (b * x * z, -b * y * z, f(0.5) * b * (xx - yy))
        D[15] = (f(3.0) * a * (xx - yy), -f(6.0) * a * x * y, 0)
    return D


def _sum(x, order, dtype):
    """the sum of x over axis 0 in `dtype`, one rounding per addition, in the given order"""
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:], dtype=dtype)
    return np.cumsum(x[order] if order is not None else x, axis=0, dtype=dtype)[-1]


def ray_gradients(sigma, coefficients, lo, hi, origins, directions, near, far, step, target, support, white_background=False,
                  termination=0.0, dtype=np.float64, order=None, n_norm=None, info=None, rays64=False):
    """(L, grad_origin [N,3], grad_direction [N,3]) of L = (1 / 3 N) sum_rays sum_c (out_c - target_c)^2, all arithmetic in `dtype`;
    the arguments are those of baked_train_reference.loss_and_grad.  order: a numpy Generator; every ray's sums over its samples are
    then formed in a random order (default: ascending).  rays64: origins and directions are taken as float64 values as they are
    (the central differences of the host tests move a ray by less than a float32 can hold); default: rounded to float32 first, as
    the kernels receive them.  info: a dict that receives per ray
      "cell_margin" [N]  the smallest distance, in cells, of any sample of the ray that lies in the box to an integer plane of the
                         lattice (the box faces are such planes), and of any sample outside the box to the box: what a rounding
                         error of the lattice coordinate must stay below for the sample to keep its cell (inf: no sample);
      "end_margin" [N]   the distance of (far - near) / step from an integer, in samples: below it the ray's sample count is the same;
      "clamp_margin" [N] the smallest distance of a fetched sample's raw colour channel, and of the output before its clamp (rays with
                         opacity > 0), from 0 and 1 (inf: nothing fetched);
      "term_margin" [N]  with termination: the smallest |T / termination - 1| over the transmittances behind the ray's fetched samples
                         (inf: none);
      "fetched" [N]      the number of samples fetched;  "opacity" [N]."""
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
    o_all = np.asarray(origins, dtype=np.float64 if rays64 else np.float32).astype(f)
    d_all = np.asarray(directions, dtype=np.float64 if rays64 else np.float32).astype(f)
    tg = np.asarray(target, dtype=np.float32).astype(f)
    N = o_all.shape[0]
    norm = f(N if n_norm is None else n_norm)
    near = np.broadcast_to(np.asarray(near, dtype=np.float32), (N,)).astype(f)
    far = np.broadcast_to(np.asarray(far, dtype=np.float32), (N,)).astype(f)
    h = f(np.float32(step))
    eps = f(np.float32(termination))
    bg = f(1.0 if white_background else 0.0)
    sg_flat, co_flat = sg.reshape(-1), co.reshape(-1, K, 3)
    g_o, g_d = np.zeros((N, 3), dtype=f), np.zeros((N, 3), dtype=f)
    cell_margin, end_margin, clamp_margin, term_margin = (np.full(N, np.inf) for _ in range(4))
    fetched, opacity = np.zeros(N, dtype=np.int64), np.zeros(N)
    sq_total = 0.0
    for r in range(N):
        o, d = o_all[r], d_all[r]
        q = (np.float64(far[r]) - np.float64(near[r])) / np.float64(h)
        S = max(int(np.ceil(q)), 0)
        end_margin[r] = abs(q - np.round(q))
        nrm = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        unit = d / nrm if nrm > 0 else np.zeros(3, dtype=f)
        Y = R.real_sh(unit, degree, dtype=f)
        t = near[r] + (np.arange(S, dtype=f) + f(0.5)) * h
        p = o[None, :] + d[None, :] * t[:, None]
        u = (p - lo[None, :]) * scale[None, :]
        inside = np.all((u >= 0) & (u <= cells[None, :]), axis=1)
        if S:
            u64 = u.astype(np.float64)
            out_dist = np.maximum(np.maximum(-u64, u64 - cells[None, :].astype(np.float64)), 0).max(axis=1)
            plane = np.abs(u64 - np.round(u64)).min(axis=1)
            cell_margin[r] = float(np.where(inside, plane, out_dist).min())
        ui, ti = u[inside], t[inside]
        cell = np.minimum(np.floor(ui), cells[None, :] - 1).astype(np.int64)
        keep = support[cell[:, 0], cell[:, 1], cell[:, 2]]
        ui, cell, ti = ui[keep], cell[keep], ti[keep]
        fr = ui - cell.astype(f)
        M = cell.shape[0]
        tau, dtau = np.zeros((M, 8), dtype=f), np.zeros((M, 8, 3), dtype=f)
        idx = np.zeros((M, 8), dtype=np.int64)
        n_ = 0
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    wx, wy, wz = (fr[:, 0] if a else 1 - fr[:, 0]), (fr[:, 1] if b else 1 - fr[:, 1]), (fr[:, 2] if c else 1 - fr[:, 2])
                    tau[:, n_] = wx * wy * wz
                    dtau[:, n_, 0] = (wy * wz) * f(1 if a else -1)
                    dtau[:, n_, 1] = (wx * wz) * f(1 if b else -1)
                    dtau[:, n_, 2] = (wx * wy) * f(1 if c else -1)
                    idx[:, n_] = ((cell[:, 0] + a) * Rr[1] + (cell[:, 1] + b)) * Rr[2] + (cell[:, 2] + c)
                    n_ += 1
        sig_n, co_n = sg_flat[idx], co_flat[idx]                           # [M,8], [M,8,K,3]
        s_j = np.einsum("mn,mn->m", tau, sig_n).astype(f)
        c_j = np.einsum("mn,mnkc->mkc", tau, co_n).astype(f)
        raw = np.einsum("mkc,k->mc", c_j, Y).astype(f)
        delta = h * nrm
        alpha = (1 - np.exp(-(s_j * delta))).astype(f)
        Tn = np.cumprod(1 - alpha, dtype=f)                                 # T_{j+1}, in ascending sample order
        if eps > 0 and Tn.size:
            below = np.nonzero(Tn < eps)[0]
            upto = below[0] + 1 if below.size else Tn.size
            term_margin[r] = float(np.abs(Tn[:upto].astype(np.float64) / float(eps) - 1.0).min())
            if below.size:                                                  # the first sample behind which T < eps is the last one
                M = below[0] + 1
                tau, dtau, raw, alpha, Tn, ti, s_j, c_j, sig_n, co_n = (x[:M] for x in (tau, dtau, raw, alpha, Tn, ti, s_j, c_j, sig_n, co_n))
        fetched[r] = M
        Tb = np.concatenate([np.ones(1, dtype=f), Tn[:-1]]) if Tn.size else Tn
        w = (Tb * alpha).astype(f)
        col = np.clip(raw, 0, 1)
        C = np.cumsum(w[:, None] * col, axis=0, dtype=f)[-1] if w.size else np.zeros(3, dtype=f)
        O = np.cumsum(w, dtype=f)[-1] if w.size else f(0)
        pre = C + bg * (1 - O)
        out = np.clip(pre, 0, 1)
        opacity[r] = float(O)
        diff = out - tg[r]
        sq_total += float(np.sum(diff.astype(np.float64) ** 2)) if f is np.float64 else float(np.sum(diff * diff, dtype=f))
        if not w.size:
            continue
        cm = min(float(np.abs(raw).min()), float(np.abs(raw - 1).min()))
        if O > 0:
            cm = min(cm, float(np.abs(pre).min()), float(np.abs(pre - 1).min()))
        clamp_margin[r] = cm
        if not nrm > 0:
            continue
        g = (f(2) * diff / (f(3) * norm)) * ((pre >= 0) & (pre <= 1))
        dr = g[None, :] * w[:, None] * ((raw >= 0) & (raw <= 1))
        A = ((col - bg) * g[None, :]).sum(axis=1).astype(f)
        wA = w * A
        later = np.concatenate([np.cumsum(wA[::-1], dtype=f)[::-1][1:], np.zeros(1, dtype=f)])     # sum over i > j
        ds = delta * (Tn * A - later)
        # the field's spatial gradient in the cell, by the lattice coordinate: 8 differences
        r_n = np.einsum("mnkc,k->mnc", co_n, Y).astype(f)                   # the colour of each corner alone
        dsig_dfr = np.einsum("mna,mn->ma", dtau, sig_n).astype(f)
        draw_dfr = np.einsum("mna,mnc->mac", dtau, r_n).astype(f)
        G = (scale[None, :] * (ds[:, None] * dsig_dfr + np.einsum("mc,mac->ma", dr, draw_dfr))).astype(f)
        perm = order.permutation(M) if order is not None else None
        g_o[r] = _sum(G, perm, f)
        # the direction also stretches the samples (delta = step |d|) and turns the basis
        stretch = _sum(ds * s_j, perm, f) * (h / delta)
        Q = _sum(dr[:, None, :] * c_j, perm, f)                             # [K,3]: sum_j dr_jc cf_jkc
        vy = np.einsum("kc,ka->a", Q, real_sh_grad(unit, degree, dtype=f)).astype(f)
        g_d[r] = _sum(ti[:, None] * G, perm, f) + stretch * unit + (vy - unit * np.dot(unit, vy)) / nrm
    if info is not None:
        info.update(cell_margin=cell_margin, end_margin=end_margin, clamp_margin=clamp_margin, term_margin=term_margin, fetched=fetched,
                    opacity=opacity)
    return sq_total / (3.0 * float(norm)), g_o, g_d


# ---- from rays to cameras
def pose_gradients(grad_origin, grad_direction, directions, view, n_views):
    """[V,6] float64: per view the sum of grad_origin (tau) and of directions x grad_direction (omega) over its rays, the derivative at
    0 of R <- exp(omega^) R, t <- t + tau for rays o = t, d = R cam.  A view index outside [0, V) is skipped."""
    go, gd, d = (np.asarray(x, dtype=np.float64) for x in (grad_origin, grad_direction, directions))
    view = np.asarray(view).astype(np.int64)
    out = np.zeros((int(n_views), 6))
    ok = (view >= 0) & (view < int(n_views))
    np.add.at(out[:, :3], view[ok], go[ok])
    np.add.at(out[:, 3:], view[ok], np.cross(d[ok], gd[ok]))
    return out


def rodrigues(omega):
    """exp(omega^) for omega [..., 3] in float64: I + sin(th)/th K + (1 - cos th)/th^2 K^2, with the series' first terms below th = 1e-4"""
    w = np.asarray(omega, dtype=np.float64)
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    Kx = np.zeros(w.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2] = -w[..., 2], w[..., 1]
    Kx[..., 1, 0], Kx[..., 1, 2] = w[..., 2], -w[..., 0]
    Kx[..., 2, 0], Kx[..., 2, 1] = -w[..., 1], w[..., 0]
    small = th < 1e-4
    safe = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6.0, np.sin(safe) / safe)
    b = np.where(small, 0.5 - th * th / 24.0, (1.0 - np.cos(safe)) / (safe * safe))
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def move_poses(c2w, omega, tau):
    """the poses [V,4,4] (float64) after R <- exp(omega^) R, t <- t + tau"""
    out = np.array(c2w, dtype=np.float64)
    out[:, :3, :3] = rodrigues(omega) @ out[:, :3, :3]
    out[:, :3, 3] += np.asarray(tau, dtype=np.float64)
    return out


def pose_adam_step(c2w, m, v, grad, lr_rotation, lr_translation, beta_1, beta_2, epsilon, t, fixed=None):
    """One Keras-form Adam step on the [V,6] rigid-motion gradient (tau first, then omega), t the step applied (from 1), in float64:
    m += (g - m)(1 - b1), v += (g g - v)(1 - b2), step = lr_t m / (sqrt(v) + eps), lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) with
    lr_translation for tau and lr_rotation for omega; then R <- exp(-step_omega^) R, t <- t - step_tau.  Views in `fixed` (bool [V])
    keep pose and moments.  Returns (c2w, m, v) in float64; the product stores the poses as float32."""
    c2w, m, v, g = (np.array(x, dtype=np.float64) for x in (c2w, m, v, grad))
    V = c2w.shape[0]
    move = np.ones(V, dtype=bool) if fixed is None else ~np.asarray(fixed, dtype=bool)
    corr = np.sqrt(1.0 - float(beta_2) ** t) / (1.0 - float(beta_1) ** t)
    rate = np.array([lr_translation * corr] * 3 + [lr_rotation * corr] * 3)
    m2 = m + (g - m) * (1.0 - beta_1)
    v2 = v + (g * g - v) * (1.0 - beta_2)
    step = rate[None, :] * m2 / (np.sqrt(v2) + epsilon)
    step = np.where(move[:, None], step, 0.0)
    out = move_poses(c2w, -step[:, 3:], -step[:, :3])
    out[~move] = c2w[~move]
    return out, np.where(move[:, None], m2, m), np.where(move[:, None], v2, v)
