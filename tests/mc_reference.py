"""NumPy reference of csrc/mesh.hip (marching cubes): the same table (keras_nerf_amd/mesh_table.py), lattice, edge ids, vertex and
normal formulas, in float32 with the kernel's operation order; plus the mesh checks the tests share."""
import numpy as np

from keras_nerf_amd import mesh_table as MT

f32 = np.float32


def lattice(resolution, lo, hi):
    """per axis: float32 coordinates lo + idx * step, step = (hi - lo) / (R - 1) in float32 (csrc/query.hip, csrc/mesh.hip)"""
    out = []
    for r, l, h in zip(resolution, lo, hi):
        step = (f32(h) - f32(l)) / f32(r - 1)
        out.append(f32(l) + np.arange(r).astype(f32) * step)
    return out


def steps(resolution, lo, hi):
    return [(f32(h) - f32(l)) / f32(r - 1) for r, l, h in zip(resolution, lo, hi)]


def grid_points(resolution, lo, hi):
    """[R0 R1 R2, 3] float32 points of the grid, C order"""
    ax = lattice(resolution, lo, hi)
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return np.stack([X, Y, Z], -1).reshape(-1, 3)


def _grad(s, st):
    """per axis b: d sigma / d x_b at every point (central differences, one-sided at the border), float32 as the kernel"""
    g = []
    for b in range(3):
        d = np.empty_like(s)
        R = s.shape[b]
        sl = lambda a, z: tuple(slice(a, z) if k == b else slice(None) for k in range(3))
        d[sl(1, R - 1)] = (s[sl(2, R)] - s[sl(0, R - 2)]) / (f32(2) * st[b])
        d[sl(0, 1)] = (s[sl(1, 2)] - s[sl(0, 1)]) / (f32(1) * st[b])
        d[sl(R - 1, R)] = (s[sl(R - 1, R)] - s[sl(R - 2, R - 1)]) / (f32(1) * st[b])
        g.append(d.reshape(-1))
    return g


def marching_cubes(sigma, tau, lo, hi):
    s = np.ascontiguousarray(sigma, dtype=f32)
    R = s.shape
    tau = f32(tau)
    inside = s > tau
    n = s.size
    strides = (R[1] * R[2], R[2], 1)
    flags = np.zeros((n, 3), bool)
    for a in range(3):
        m = np.zeros(R, bool)
        sl0 = tuple(slice(0, R[k] - 1) if k == a else slice(None) for k in range(3))
        sl1 = tuple(slice(1, R[k]) if k == a else slice(None) for k in range(3))
        m[sl0] = inside[sl0] != inside[sl1]
        flags[:, a] = m.reshape(-1)
    flags = flags.reshape(-1)
    vid = np.cumsum(flags) - flags
    e = np.nonzero(flags)[0]
    p, a = e // 3, e % 3
    q = p + np.array(strides)[a]
    sf = s.reshape(-1)
    sa, sb = sf[p], sf[q]
    t = (tau - sa) / (sb - sa)
    ax = lattice(R, lo, hi)
    idx = np.stack(np.unravel_index(p, R), -1)
    verts = np.empty((e.size, 3), f32)
    for b in range(3):
        pa = ax[b][idx[:, b]]
        pb = ax[b][np.minimum(idx[:, b] + 1, R[b] - 1)]
        verts[:, b] = np.where(a == b, pa + t * (pb - pa), pa)
    g = _grad(s, steps(R, lo, hi))
    u = f32(1) - t
    nrm = np.stack([-(u * g[b][p] + t * g[b][q]) for b in range(3)], -1).astype(f32)
    ln = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    nrm = np.where(ln[:, None] > 0, nrm / np.where(ln > 0, ln, f32(1))[:, None], f32(0)).astype(f32)
    # cubes: corner 0 at point p
    counts, tris = MT.table()
    ins = inside.astype(np.int32)
    case = np.zeros((R[0] - 1, R[1] - 1, R[2] - 1), np.int32)
    for c in range(8):
        x, y, z = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[x:R[0] - 1 + x, y:R[1] - 1 + y, z:R[2] - 1 + z] << c
    cp = np.stack(np.meshgrid(*[np.arange(r - 1) for r in R], indexing="ij"), -1).reshape(-1, 3) @ np.array(strides)
    case = case.reshape(-1)
    cnt = counts[case].astype(np.int64)
    off = np.cumsum(cnt) - cnt
    faces = np.empty((int(cnt.sum()), 3), np.int32)
    corner_off = np.array([(c & 1) * strides[0] + ((c >> 1) & 1) * strides[1] + ((c >> 2) & 1) for c in range(8)])
    for k in range(tris.shape[1]):
        m = cnt > k
        ce = tris[case[m], k].astype(np.int64)                     # [m, 3] cube edges
        c0 = np.array([ed[0] for ed in MT.EDGES])[ce]
        axis = np.array([ed[2] for ed in MT.EDGES])[ce]
        ge = 3 * (cp[m][:, None] + corner_off[c0]) + axis
        faces[off[m] + k] = vid[ge]
    return verts, faces, nrm


def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def check_closed_manifold(faces, n_verts):
    """every directed edge exactly once and its reverse exactly once (closed, consistently oriented edge-manifold), no repeated index"""
    f = np.asarray(faces, np.int64)
    assert f.size, "empty mesh"
    assert np.all((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])), "a face repeats an index"
    de = directed_edges(f)
    key = de[:, 0] * n_verts + de[:, 1]
    u, c = np.unique(key, return_counts=True)
    assert c.max() == 1, "a directed edge is used twice (inconsistent orientation or non-manifold edge)"
    rev = de[:, 1] * n_verts + de[:, 0]
    assert np.isin(rev, u).all(), "an edge without its reverse (open boundary)"


def euler(faces, n_verts):
    de = directed_edges(faces)
    n_edges = np.unique(np.sort(de, 1)[:, 0] * n_verts + np.sort(de, 1)[:, 1]).size
    used = np.unique(np.asarray(faces).reshape(-1)).size
    return used - n_edges + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def sphere(res, r=1.0, c=(0.0, 0.0, 0.0), lo=(-1.5,) * 3, hi=(1.5,) * 3):
    P = grid_points((res,) * 3, lo, hi).astype(np.float64) - np.array(c)
    return (r - np.linalg.norm(P, axis=1)).reshape((res,) * 3).astype(f32)


def torus(res, R=0.8, r=0.3, lo=(-1.5,) * 3, hi=(1.5,) * 3):
    P = grid_points((res,) * 3, lo, hi).astype(np.float64)
    q = np.sqrt(P[:, 0] ** 2 + P[:, 1] ** 2) - R
    return (r - np.sqrt(q ** 2 + P[:, 2] ** 2)).reshape((res,) * 3).astype(f32)
