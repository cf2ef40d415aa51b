"""fp64 restatement of the point query of a baked field, written from the specification in include/knerf.h (knerf_baked_query), not
from the kernel.

The cell lookup is a float32 NumPy mirror: one subtraction, one multiplication and one floor per axis, each rounded once, which
NumPy's float32 arithmetic reproduces exactly -- so the reference and the kernel agree on the cell and on the fractions bit for bit, and
only the interpolation remains to be compared.  Weights, sums, the SH basis and the gradient are computed in float64 from those float32
fractions.  For every output the sum of the absolute values of its terms comes back as well: the rounding bound of
tests/README_baked_query.md scales with it.
"""
import numpy as np

from keras_nerf_amd.baked import sh_basis

U = 2.0 ** -24          # the unit roundoff of fp32


def lattice_scale(resolution, lo, hi):
    """fp32(cells / (hi - lo)) computed in double from the fp32 box, per axis"""
    lo32, hi32 = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    cells = np.asarray(resolution, dtype=np.float64) - 1.0
    return (cells / (hi32.astype(np.float64) - lo32.astype(np.float64))).astype(np.float32)


def locate(points, resolution, lo, hi):
    """float32 mirror of the cell lookup: (inside bool [n], cell int64 [n,3], fractions float32 [n,3])"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    lo32 = np.asarray(lo, dtype=np.float32)
    scale = lattice_scale(resolution, lo, hi)
    cells = np.asarray(resolution, dtype=np.int64) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((p - lo32).astype(np.float32) * scale).astype(np.float32)
        ok = (u >= 0) & (u <= cells.astype(np.float32))                       # NaN fails both
        f = np.where(ok, np.floor(np.where(ok, u, 0)), 0).astype(np.int64)
        cell = np.minimum(f, cells - 1)
        fr = (u - cell.astype(np.float32)).astype(np.float32)
    return ok.all(axis=1), cell, fr


def grid_points(resolution, lo, hi):
    """the points of grid mode in float32, by the stated two roundings: lo + fp32(idx * step), step = (hi - lo) / (R - 1) in fp32;
    [Rx Ry Rz, 3] in C order, z fastest"""
    lo32, hi32 = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    axes = []
    for c in range(3):
        step = np.float32(np.float32(hi32[c] - lo32[c]) / np.float32(resolution[c] - 1))
        axes.append((lo32[c] + (np.arange(resolution[c], dtype=np.float32) * step).astype(np.float32)).astype(np.float32))
    g = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
    return np.ascontiguousarray(g.reshape(-1, 3), dtype=np.float32)


def direction_seen(d):
    """float32 mirror of the decision whether a direction has a usable length: |d| = sqrt(dx dx + dy dy + dz dz), every operation
    rounded once; usable iff 0 < |d| < inf"""
    d = np.asarray(d, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = ((d[:, 0] * d[:, 0]).astype(np.float32) + (d[:, 1] * d[:, 1]).astype(np.float32)).astype(np.float32)
        s = (s + (d[:, 2] * d[:, 2]).astype(np.float32)).astype(np.float32)
        nrm = np.sqrt(s).astype(np.float32)
        return (nrm > 0) & np.isfinite(nrm)


def sh_basis_abs(unit, sh_degree):
    """sh_basis with every monomial of every Y_k taken by its absolute value, [..., K]: the sum of the absolute values of a basis
    value's own terms (Y_6 = b (3 zz - 1) vanishes on a cone, its rounding error does not)"""
    v = np.abs(np.asarray(unit, dtype=np.float64))
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    pi = np.pi
    Y = [np.full(x.shape, 0.5 / np.sqrt(pi))]
    if sh_degree >= 1:
        c = np.sqrt(3.0 / (4.0 * pi))
        Y += [c * y, c * z, c * x]
    if sh_degree >= 2:
        a, b = 0.5 * np.sqrt(15.0 / pi), 0.25 * np.sqrt(5.0 / pi)
        Y += [a * x * y, a * y * z, b * (3.0 * z * z + 1.0), a * x * z, 0.5 * a * (x * x + y * y)]
    if sh_degree >= 3:
        a, b = 0.25 * np.sqrt(35.0 / (2.0 * pi)), 0.5 * np.sqrt(105.0 / pi)
        c, d = 0.25 * np.sqrt(21.0 / (2.0 * pi)), 0.25 * np.sqrt(7.0 / pi)
        Y += [a * y * (3.0 * x * x + y * y), b * x * y * z, c * y * (5.0 * z * z + 1.0), d * z * (5.0 * z * z + 3.0),
              c * x * (5.0 * z * z + 1.0), 0.5 * b * z * (x * x + y * y), a * x * (x * x + 3.0 * y * y)]
    return np.stack(Y, axis=-1)


def query(sigma, coefficients, lo, hi, points, directions=None):
    """sigma [Rx,Ry,Rz], coefficients [Rx,Ry,Rz,K,3] (the stored values), points [n,3] float32, directions None, [3] or [n,3] ->
    dict of float64 arrays: sigma [n], rgb [n,3] (clamped), grad [n,3], their term sums sigma_abs, rgb_abs, grad_abs, and inside [n]"""
    sg = np.asarray(sigma, dtype=np.float64)
    co = np.asarray(coefficients, dtype=np.float64)
    res = sg.shape
    K = co.shape[3]
    deg = int(round(np.sqrt(K))) - 1
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    inside, cell, fr32 = locate(p, res, lo, hi)
    fr = np.where(inside[:, None], fr32.astype(np.float64), 0.0)        # (outside everything is 0 whatever the fractions are)
    scale = lattice_scale(res, lo, hi).astype(np.float64)
    # the SH basis of the normalised direction; the DC term alone without a usable direction
    Y, Y_abs = np.zeros((n, K)), np.zeros((n, K))
    Y[:, 0] = Y_abs[:, 0] = sh_basis(np.zeros((1, 3)), 0)[0, 0]
    if directions is not None:
        d = np.broadcast_to(np.asarray(directions, dtype=np.float32).reshape(-1, 3), (n, 3)).astype(np.float64)
        seen = direction_seen(np.broadcast_to(np.asarray(directions, dtype=np.float32).reshape(-1, 3), (n, 3)))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            unit = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
        Y[seen] = sh_basis(unit[seen], deg)
        Y_abs[seen] = sh_basis_abs(unit[seen], deg)
    out = {k: np.zeros((n,) + s) for k, s in (("sigma", ()), ("sigma_abs", ()), ("rgb", (3,)), ("rgb_abs", (3,)), ("grad", (3,)),
                                               ("grad_abs", (3,)))}
    w1 = np.stack([1.0 - fr, fr], axis=1)                   # [n, 2, 3]: the one-axis weights, lower / upper
    cs = np.zeros((n, 8))                                   # the corner sigmas
    cf, cf_abs = np.zeros((n, K, 3)), np.zeros((n, K, 3))
    for cn in range(8):
        bx, by, bz = (cn >> 2) & 1, (cn >> 1) & 1, cn & 1
        ix, iy, iz = cell[:, 0] + bx, cell[:, 1] + by, cell[:, 2] + bz
        w = w1[:, bx, 0] * w1[:, by, 1] * w1[:, bz, 2]
        cs[:, cn] = sg[ix, iy, iz]
        out["sigma"] += w * cs[:, cn]
        out["sigma_abs"] += np.abs(w * cs[:, cn])
        c = co[ix, iy, iz]
        cf += w[:, None, None] * c
        cf_abs += np.abs(w[:, None, None] * c)
    rgb = (cf * Y[:, :, None]).sum(axis=1)
    out["rgb"] = np.clip(rgb, 0.0, 1.0)
    out["rgb_abs"] = (cf_abs * Y_abs[:, :, None]).sum(axis=1)
    for ax in range(3):
        bit = 4 >> ax
        b, c = [a for a in range(3) if a != ax]
        for cn in range(8):
            if cn & bit:
                continue
            wb, wc = w1[:, (cn >> (2 - b)) & 1, b], w1[:, (cn >> (2 - c)) & 1, c]
            out["grad"][:, ax] += wb * wc * (cs[:, cn | bit] - cs[:, cn])
            out["grad_abs"][:, ax] += np.abs(wb * wc) * (np.abs(cs[:, cn | bit]) + np.abs(cs[:, cn]))
        out["grad"][:, ax] *= scale[ax]
        out["grad_abs"][:, ax] *= scale[ax]
    for k in out:
        out[k][~inside] = 0.0
    out["inside"] = inside
    return out


def roundings(output, sh_degree=0):
    """the number of fp32 roundings on the path of one term of an output (tests/README_baked_query.md writes the count out)"""
    K = (sh_degree + 1) ** 2
    return {"sigma": 3 + 8, "rgb": 3 + 8 + 3 * K, "grad": 3 + 1 + 4 + 1}[output]


def bound(output, abs_sum, sh_degree=0):
    """2 x roundings x 2^-24 x the sum of the absolute values of the output's terms"""
    return 2.0 * roundings(output, sh_degree) * U * np.asarray(abs_sum, dtype=np.float64)
