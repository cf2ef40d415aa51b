"""NumPy reference of csrc/mesh.hip (marching cubes): the same table (keras_nerf_amd/mesh_table.py), lattice, edge ids, vertex and
normal formulas, in float32 with the kernel's operation order, and in float64 on the same float32 grid and classification; four
deliberate mutants of it; the mesh checks and the table of edge-case grids the tests share."""
import functools

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


SCAN_BLOCK = 1024                                       # csrc/mesh.hip kScanBlock: elements per block of the device's exclusive scan
MUTANTS = ("ge", "scan", "two_sided", "far_t")          # deliberate one-line errors (tests/test_mesh_edges_host.py): see marching_cubes


def lattice64(resolution, lo, hi):
    """the same lattice from the same float32 lo / hi, step and coordinates in float64"""
    out = []
    for r, l, h in zip(resolution, lo, hi):
        l, h = np.float64(f32(l)), np.float64(f32(h))
        out.append(l + np.arange(r).astype(np.float64) * ((h - l) / np.float64(r - 1)))
    return out


def _grad(s, st, two_sided=False):
    """per axis b: d sigma / d x_b at every point (central differences, one-sided at the border), in s.dtype with the kernel's
    operation order.  two_sided (a mutant): the border difference divided by two steps as well"""
    g = []
    dt = s.dtype.type
    for b in range(3):
        d = np.empty_like(s)
        R = s.shape[b]
        sl = lambda a, z: tuple(slice(a, z) if k == b else slice(None) for k in range(3))
        border = dt(2 if two_sided else 1) * dt(st[b])
        d[sl(1, R - 1)] = (s[sl(2, R)] - s[sl(0, R - 2)]) / (dt(2) * dt(st[b]))
        d[sl(0, 1)] = (s[sl(1, 2)] - s[sl(0, 1)]) / border
        d[sl(R - 1, R)] = (s[sl(R - 1, R)] - s[sl(R - 2, R - 1)]) / border
        g.append(d.reshape(-1))
    return g


@functools.lru_cache(None)
def _table():
    return MT.table()


def _exclusive_scan(x, mutant):
    c = np.cumsum(x) - x
    if mutant == "scan":                                 # the offset of every block but the first dropped
        c = c - c[(np.arange(x.size) // SCAN_BLOCK) * SCAN_BLOCK]
    return c


def _geometry(s32, tau, lo, hi, e, dt, mutant):
    """vertices, normals and the un-normalised normal's length of the crossed edges e, computed in dt on the float32 samples"""
    R = s32.shape
    strides = np.array((R[1] * R[2], R[2], 1))
    s = s32.astype(dt)
    tau = dt(tau)
    p, a = e // 3, e % 3
    q = p + strides[a]
    sf = s.reshape(-1)
    sa, sb = sf[p], sf[q]
    t = (tau - sb) / (sa - sb) if mutant == "far_t" else (tau - sa) / (sb - sa)
    if dt is f32:
        ax, st = lattice(R, lo, hi), steps(R, lo, hi)
    else:
        ax = lattice64(R, lo, hi)
        st = [(np.float64(f32(h)) - np.float64(f32(l))) / np.float64(r - 1) for r, l, h in zip(R, lo, hi)]
    idx = np.stack(np.unravel_index(p, R), -1)
    verts = np.empty((e.size, 3), dt)
    for b in range(3):
        pa = ax[b][idx[:, b]]
        pb = ax[b][np.minimum(idx[:, b] + 1, R[b] - 1)]
        verts[:, b] = np.where(a == b, pa + t * (pb - pa), pa)
    g = _grad(s, st, mutant == "two_sided")
    u = dt(1) - t
    nrm = np.stack([-(u * g[b][p] + t * g[b][q]) for b in range(3)], -1).astype(dt)
    ln = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    nrm = np.where(ln[:, None] > 0, nrm / np.where(ln > 0, ln, dt(1))[:, None], dt(0)).astype(dt)
    return verts, nrm, ln


def marching_cubes(sigma, tau, lo, hi, dtype=f32, mutant=None, details=False):
    """dtype float32: the kernel's mirror, operation by operation.  dtype float64: the same float32 grid and the same classification
    (so the same faces) with lattice coordinates, interpolation parameter, gradients and normalisation in float64.
    dtype a tuple: the classification once, (vertices, faces, normals) per entry.
    mutant: one of MUTANTS -- `>=` for `>`; the scan offset dropped for every scan block but the first; a two-sided gradient at the
    border; t taken from the far end.  details: also a dict with the crossed edge ids (vertex v lies on edge e[v] = 3 point + axis),
    the un-normalised normals' lengths per dtype and the cube cases."""
    assert mutant is None or mutant in MUTANTS
    s = np.ascontiguousarray(sigma, dtype=f32)
    R = s.shape
    tau = f32(tau)
    with np.errstate(invalid="ignore"):
        inside = s >= tau if mutant == "ge" else s > tau
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
    vid = _exclusive_scan(flags.astype(np.int64), mutant)
    e = np.nonzero(flags)[0]
    dts = dtype if isinstance(dtype, tuple) else (dtype,)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        geo = [_geometry(s, tau, lo, hi, e, np.dtype(d).type, mutant) for d in dts]
    # cubes: corner 0 at point p
    counts, tris = _table()
    ins = inside.astype(np.int32)
    case = np.zeros((R[0] - 1, R[1] - 1, R[2] - 1), np.int32)
    for c in range(8):
        x, y, z = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[x:R[0] - 1 + x, y:R[1] - 1 + y, z:R[2] - 1 + z] << c
    cp = np.stack(np.meshgrid(*[np.arange(r - 1) for r in R], indexing="ij"), -1).reshape(-1, 3) @ np.array(strides)
    case = case.reshape(-1)
    cnt_all = np.zeros(n, np.int64)                                 # per POINT, as the device scans it (border points count 0)
    cnt_all[cp] = counts[case]
    off = _exclusive_scan(cnt_all, mutant)[cp]
    cnt = cnt_all[cp]
    faces = np.empty((int(cnt.sum()), 3), np.int32)
    corner_off = np.array([(c & 1) * strides[0] + ((c >> 1) & 1) * strides[1] + ((c >> 2) & 1) for c in range(8)])
    for k in range(tris.shape[1]):
        m = cnt > k
        ce = tris[case[m], k].astype(np.int64)                     # [m, 3] cube edges
        c0 = np.array([ed[0] for ed in MT.EDGES])[ce]
        axis = np.array([ed[2] for ed in MT.EDGES])[ce]
        ge = 3 * (cp[m][:, None] + corner_off[c0]) + axis
        faces[off[m] + k] = vid[ge]
    out = [(v, faces, nm) for v, nm, _ in geo]
    out = tuple(out) if isinstance(dtype, tuple) else out[0]
    if details:
        return out, {"edges": e, "lengths": [ln for _, _, ln in geo], "cases": case}
    return out


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


# ---- the grids of tests/test_gpu_mesh_edges.py and tests/test_mesh_edges_host.py: name -> (maker, tau); lo / hi = -1.5 / 1.5

def noise(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape).astype(f32)


def one_corner():
    s = np.full((2, 2, 2), -1, f32)
    s[0, 0, 0] = 1
    return s


def corner_pattern(case):
    """the 2x2x2 grid (values +-1) whose only cube is table row `case`: corner k = (k & 1, k >> 1 & 1, k >> 2 & 1) inside when bit k is set"""
    s = np.empty((2, 2, 2), f32)
    for k in range(8):
        s[k & 1, (k >> 1) & 1, (k >> 2) & 1] = 1 if (case >> k) & 1 else -1
    return s


def checkerboard(shape):
    i, j, k = np.meshgrid(*[np.arange(r) for r in shape], indexing="ij")
    return np.where((i + j + k) % 2 == 0, 1, -1).astype(f32)


def integers(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 3, shape).astype(f32)


def padded(s, value=-1):
    return np.pad(s, 1, constant_values=value).astype(f32)


EDGE_GRIDS = {
    "one_corner": (one_corner, 0.0),                                  # one scan block, both totals through the single-block path
    "noise_5x5x41": (lambda: noise((5, 5, 41)), 0.0),                 # N = 1,025: cube scan 1,024 + 1, edge scan 3 x 1,024 + 3
    "noise_8x8x16": (lambda: noise((8, 8, 16)), 0.0),                 # N = 1,024: exactly one / exactly three full blocks
    "noise_17": (lambda: noise((17, 17, 17)), 0.0),                   # all 256 cases
    "noise_17_padded": (lambda: padded(noise((17, 17, 17))), 0.0),    # the same inside one layer of -1: a closed surface
    "noise_71": (lambda: noise((71, 71, 71)), 0.0),                   # 3N = 1,073,733: 1,049 -> 2 -> 1 blocks
    "noise_1025x32x32": (lambda: noise((1025, 32, 32)), 0.0),         # N = 1,049,600: 1,025 -> 2 -> 1 blocks for the cube scan too
    "checkerboard_24x23x22": (lambda: checkerboard((24, 23, 22)), 0.0),
    "integers_20x21x22": (lambda: integers((20, 21, 22)), 1.0),       # samples exactly on the threshold
    "slab_2x64x64": (lambda: noise((2, 64, 64)), 0.0),
    "slab_64x2x64": (lambda: noise((64, 2, 64)), 0.0),
    "slab_64x64x2": (lambda: noise((64, 64, 2)), 0.0),
    "all_inside": (lambda: np.ones((6, 7, 9), f32), 0.0),
    "all_outside": (lambda: -np.ones((6, 7, 9), f32), 0.0),
}
LARGE_GRIDS = ("noise_71", "noise_1025x32x32")
NORMAL_FLOOR, NORMAL_CAP = 1e-3, 0.03


def comparable_normals(lengths64):
    """which normals are compared with the float64 form: those whose float64 un-normalised length is above NORMAL_FLOOR x the case's
    median length (below it the direction is rounding noise in float32), and those whose length is exactly zero: there the float64
    normal is defined as exactly zero, the mirror's is too, and the device's must be (on the checkerboard that is most of them)."""
    ln = np.asarray(lengths64, np.float64)
    if ln.size == 0:
        return np.zeros(0, bool)
    return (ln > NORMAL_FLOOR * np.median(ln)) | (ln == 0)


def float64_bounds(extent, ref32, ref64, keep):
    """the bounds of a device result against the float64 form: max(1e-6 x extent, 4 x the float32 mirror's own largest deviation)"""
    (rv, _, rn), (dv, _, dn) = ref32, ref64
    tol_v = max(1e-6 * extent, 4 * float(np.abs(rv - dv).max(initial=0)))
    tol_n = max(1e-6 * extent, 4 * float(np.abs(rn - dn)[keep].max(initial=0)))
    return tol_v, tol_n
