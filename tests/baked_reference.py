"""NumPy reference of the baked field (include/knerf.h "The baked field"), written from the specification, not from the kernel: the
orthonormal real spherical harmonics up to degree 3, the Fibonacci directions and pseudo-inverse fit of the bake, trilinear lookup
and the ray marcher.  Everything takes a dtype: float64 is the reference, float32 its own rounding error (the tests' yardstick).
"""
import numpy as np


def n_coeff(degree):
    return (degree + 1) ** 2


def real_sh(v, degree, dtype=np.float64):
    """Y_k(v), k = l (l + 1) + m, for unit vectors v [..., 3]: [..., K].  Orthonormal on the sphere, no Condon-Shortley phase:
    Y_00 = 1 / (2 sqrt pi); Y_1m = sqrt(3 / 4 pi) (y, z, x); Y_2m = (1/2 sqrt(15/pi) xy, 1/2 sqrt(15/pi) yz, 1/4 sqrt(5/pi) (3 z^2 - 1),
    1/2 sqrt(15/pi) xz, 1/4 sqrt(15/pi) (x^2 - y^2)); Y_3m = (1/4 sqrt(35/2pi) y (3x^2 - y^2), 1/2 sqrt(105/pi) xyz,
    1/4 sqrt(21/2pi) y (5z^2 - 1), 1/4 sqrt(7/pi) z (5z^2 - 3), 1/4 sqrt(21/2pi) x (5z^2 - 1), 1/4 sqrt(105/pi) z (x^2 - y^2),
    1/4 sqrt(35/2pi) x (x^2 - 3y^2))."""
    v = np.asarray(v, dtype=dtype)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    f = lambda c: dtype(c)
    pi = np.pi
    out = [np.full(x.shape, f(1.0 / (2.0 * np.sqrt(pi))), dtype=dtype)]
    if degree >= 1:
        c = f(np.sqrt(3.0 / (4.0 * pi)))
        out += [c * y, c * z, c * x]
    if degree >= 2:
        out += [f(0.5 * np.sqrt(15.0 / pi)) * (x * y), f(0.5 * np.sqrt(15.0 / pi)) * (y * z),
                f(0.25 * np.sqrt(5.0 / pi)) * (f(3.0) * z * z - f(1.0)), f(0.5 * np.sqrt(15.0 / pi)) * (x * z),
                f(0.25 * np.sqrt(15.0 / pi)) * (x * x - y * y)]
    if degree >= 3:
        out += [f(0.25 * np.sqrt(35.0 / (2.0 * pi))) * (y * (f(3.0) * x * x - y * y)), f(0.5 * np.sqrt(105.0 / pi)) * (x * y * z),
                f(0.25 * np.sqrt(21.0 / (2.0 * pi))) * (y * (f(5.0) * z * z - f(1.0))),
                f(0.25 * np.sqrt(7.0 / pi)) * (z * (f(5.0) * z * z - f(3.0))),
                f(0.25 * np.sqrt(21.0 / (2.0 * pi))) * (x * (f(5.0) * z * z - f(1.0))),
                f(0.25 * np.sqrt(105.0 / pi)) * (z * (x * x - y * y)), f(0.25 * np.sqrt(35.0 / (2.0 * pi))) * (x * (x * x - f(3.0) * y * y))]
    return np.stack(out, axis=-1)


def fibonacci_directions(n):
    """n unit vectors: z_i = 1 - (2 i + 1) / n, longitude i times the golden angle pi (3 - sqrt 5)"""
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)


def default_n_directions(degree):
    K = n_coeff(degree)
    return 1 if degree == 0 else max(4 * K, 16)


def fit_matrix(degree, n_directions=None):
    """(directions [D,3], P [K,D]): P = pinv(Y), Y [D,K] the basis at the directions; degree 0: the one zero direction, P = 1 / Y_0"""
    if degree == 0:
        return np.zeros((1, 3)), np.array([[2.0 * np.sqrt(np.pi)]])
    dirs = fibonacci_directions(default_n_directions(degree) if n_directions is None else n_directions)
    return dirs, np.linalg.pinv(real_sh(dirs, degree))


def lattice_points(resolution, lo, hi):
    """the lattice of knerf_query_grid in float32: lo + idx * step, step = (hi - lo) / (R - 1), two roundings; [Rx,Ry,Rz,3]"""
    ax = []
    for r, l, h in zip(resolution, lo, hi):
        step = (np.float32(h) - np.float32(l)) / np.float32(r - 1)
        ax.append((np.float32(l) + (np.arange(r, dtype=np.float32) * step).astype(np.float32)).astype(np.float32))
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def occupied_cells(sigma):
    """bool [Rx-1,Ry-1,Rz-1]: a cell is occupied if one of its 8 corners has sigma > 0"""
    s = np.asarray(sigma) > 0
    occ = np.zeros(tuple(r - 1 for r in s.shape), dtype=bool)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                occ |= s[a:s.shape[0] - 1 + a, b:s.shape[1] - 1 + b, c:s.shape[2] - 1 + c]
    return occ


def touched_points(occ):
    """bool [Rx,Ry,Rz]: lattice points that are a corner of at least one occupied cell"""
    t = np.zeros(tuple(c + 1 for c in occ.shape), dtype=bool)
    cx, cy, cz = occ.shape
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                t[a:a + cx, b:b + cy, c:c + cz] |= occ
    return t


def march(sigma, coefficients, lo, hi, origins, directions, near, far, step, white_background=False, termination=0.0,
          dtype=np.float64, count=None):
    """The marcher of knerf_baked_render for every ray, all arithmetic in `dtype`: image [N,3], depth [N], opacity [N].
    sigma [Rx,Ry,Rz], coefficients [Rx,Ry,Rz,K,3] (pass them already rounded to fp16), lo / hi [3], near / far scalars or [N]; the
    inputs are float32 VALUES (as the kernel receives them), `step` included.  count: a list that receives [samples with sigma looked up
    inside the box, samples of all rays]."""
    f = dtype
    sg = np.asarray(sigma, dtype=f)
    co = np.asarray(coefficients, dtype=f)
    R = np.array(sg.shape)
    K = co.shape[3]
    degree = int(round(np.sqrt(K))) - 1
    lo = np.asarray(lo, dtype=np.float32).astype(f)
    hi = np.asarray(hi, dtype=np.float32).astype(f)
    cells = (R - 1).astype(f)
    scale = (cells.astype(np.float64) / (hi.astype(np.float64) - lo.astype(np.float64))).astype(np.float32).astype(f)
    o_all = np.asarray(origins, dtype=np.float32).astype(f)
    d_all = np.asarray(directions, dtype=np.float32).astype(f)
    N = o_all.shape[0]
    near = np.broadcast_to(np.asarray(near, dtype=np.float32), (N,)).astype(f)
    far = np.broadcast_to(np.asarray(far, dtype=np.float32), (N,)).astype(f)
    h = f(np.float32(step))
    eps = f(np.float32(termination))
    image, depth, opacity = np.zeros((N, 3), dtype=f), np.zeros(N, dtype=f), np.zeros(N, dtype=f)
    inside_total, total = 0, 0
    for r in range(N):
        o, d = o_all[r], d_all[r]
        S = int(np.ceil((np.float64(far[r]) - np.float64(near[r])) / np.float64(h)))
        S = max(S, 0)
        total += S
        if S == 0:
            continue
        nrm = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        unit = d / nrm if nrm > 0 else np.zeros(3, dtype=f)
        Y = real_sh(unit, degree, dtype=f)                                  # [K]
        t = near[r] + (np.arange(S, dtype=f) + f(0.5)) * h                  # [S]
        p = o[None, :] + d[None, :] * t[:, None]                            # [S,3]
        u = (p - lo[None, :]) * scale[None, :]
        inside = np.all((u >= 0) & (u <= cells[None, :]), axis=1)
        idx = np.nonzero(inside)[0]
        inside_total += idx.size
        ui = u[idx]
        cell = np.minimum(np.floor(ui), cells[None, :] - 1).astype(np.int64)
        fr = ui - cell.astype(f)
        s_i = np.zeros(idx.size, dtype=f)
        c_i = np.zeros((idx.size, K, 3), dtype=f)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    w = (fr[:, 0] if a else 1 - fr[:, 0]) * (fr[:, 1] if b else 1 - fr[:, 1]) * (fr[:, 2] if c else 1 - fr[:, 2])
                    s_i += w * sg[cell[:, 0] + a, cell[:, 1] + b, cell[:, 2] + c]
                    c_i += w[:, None, None] * co[cell[:, 0] + a, cell[:, 1] + b, cell[:, 2] + c]
        colour = np.clip(np.einsum("skc,k->sc", c_i, Y), 0, 1).astype(f)
        alpha = (1 - np.exp(-(s_i * (h * nrm)))).astype(f)
        T = f(1.0)
        for n_, i in enumerate(idx):                                        # strictly in ascending sample order
            w = T * alpha[n_]
            image[r] += w * colour[n_]
            depth[r] += w * t[i]
            opacity[r] += w
            T = T * (1 - alpha[n_])
            if eps > 0 and T < eps:
                break
    if white_background:
        image = image + (1 - opacity)[:, None]
    if count is not None:
        count[:] = [inside_total, total]
    return np.clip(image, 0, 1), depth, opacity
