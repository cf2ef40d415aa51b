"""NumPy mirror of the occupancy grid (include/knerf.h, csrc/occupancy.hip): the cell lookup of a render sample, the bit layout, and
lattice -> cells -> dilation.  Every float operation is a separate float32 NumPy op, i.e. one rounding each, as the kernels' _rn
intrinsics."""
import numpy as np

F32 = np.float32


def scale_of(cells, lo, hi):
    """scale = fp32(c / (hi - lo)) per axis, computed in double from the fp32 box"""
    return np.array([F32(int(c) / (np.float64(F32(h)) - np.float64(F32(l)))) for c, l, h in zip(cells, lo, hi)], dtype=F32)


def ray_points(o, d, t):
    """p = o + d t of every sample [R, S, 3]: __fadd_rn(o, __fmul_rn(d, t))"""
    o, d, t = (np.asarray(x, dtype=F32) for x in (o, d, t))
    return (o[:, None, :] + (d[:, None, :] * t[..., None]).astype(F32)).astype(F32)


def lookup(p, occupied, lo, hi, outside="occupied"):
    """bool [...]: is the sample at p [..., 3] live?  u = (p - lo) * scale; outside if u < 0, floor(u) >= c or u NaN on any axis"""
    occupied = np.asarray(occupied, dtype=bool)
    cells = occupied.shape
    p = np.asarray(p, dtype=F32)
    lo32 = np.asarray(lo, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((p - lo32).astype(F32) * scale_of(cells, lo, hi)).astype(F32)
        inside = np.all((u >= 0) & (u < np.asarray(cells, dtype=F32)), axis=-1)          # NaN compares false: outside
    idx = np.where(inside[..., None], np.floor(np.where(np.isfinite(u), u, 0)), 0).astype(np.int64)
    idx = np.minimum(idx, np.asarray(cells) - 1)
    live = occupied[idx[..., 0], idx[..., 1], idx[..., 2]]
    return np.where(inside, live, outside == "occupied")


def pack(occupied):
    """bool [cx, cy, cz] -> uint32 words: bit b = (i cy + j) cz + k is bit b % 32 of word b // 32"""
    flat = np.asarray(occupied, dtype=bool).reshape(-1)
    words = np.zeros((flat.size + 31) // 32, dtype=np.uint64)
    for b in np.flatnonzero(flat):
        words[b // 32] |= np.uint64(1) << np.uint64(b % 32)
    return words.astype(np.uint32)


def corner_cells(sigma, threshold):
    """lattice [rx, ry, rz] -> bool cells [rx-1, ry-1, rz-1]: any of the 8 corners has sigma > threshold"""
    s = np.asarray(sigma, dtype=F32) > F32(threshold)
    out = np.zeros(tuple(r - 1 for r in s.shape), dtype=bool)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                out |= s[a:a + out.shape[0], b:b + out.shape[1], c:c + out.shape[2]]
    return out


def dilate(occ, d):
    """every cell within Chebyshev distance d of an occupied one (clipped to the grid)"""
    out = np.asarray(occ, dtype=bool).copy()
    for ax in range(3):
        src = out.copy()
        n = out.shape[ax]
        for k in range(1, d + 1):
            if k >= n:
                break
            lo_sl = [slice(None)] * 3; hi_sl = [slice(None)] * 3
            lo_sl[ax] = slice(0, n - k); hi_sl[ax] = slice(k, n)
            out[tuple(lo_sl)] |= src[tuple(hi_sl)]
            out[tuple(hi_sl)] |= src[tuple(lo_sl)]
    return out


def grid_from_lattice(sigma, threshold=0.0, dilation=1):
    return dilate(corner_cells(sigma, threshold), dilation)
