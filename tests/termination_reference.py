"""NumPy mirror of early ray termination (include/knerf.h "Early ray termination", csrc/termination.hip): the x factors of
compositing, the running fp32 transmittance in ascending sample order, and the cut at the first segment boundary with T < fp32(eps).
Every float operation is a separate float32 NumPy op (one rounding each); exp is NumPy's, so a factor may differ from the device's in
the last bit -- tests that compare against the GPU keep away from rays whose T lies near eps."""
import numpy as np

F32 = np.float32


def x_factors(sigma, t):
    """x [R, S]: 1 - alpha + 1e-10 with alpha = 1 - exp(-sigma delta), delta = t[i+1] - t[i], the last 1e-10 (composite.hip)"""
    sigma, t = np.asarray(sigma, F32), np.asarray(t, F32)
    delta = np.concatenate([(t[:, 1:] - t[:, :-1]).astype(F32), np.full((t.shape[0], 1), 1e-10, F32)], axis=1)
    ex = np.exp(-(sigma * delta).astype(F32)).astype(F32)
    alpha = (F32(1) - ex).astype(F32)
    return ((F32(1) - alpha).astype(F32) + F32(1e-10)).astype(F32)


def segment_length(L, S):
    """a segment longer than the pass is the whole pass"""
    return min(int(L), int(S))


def cuts(sigma, t, eps, L):
    """int64 [R]: the first terminated sample of each ray (S: none).  T = 1 in front of sample 0, then T <- T * x_i one sample at a
    time; the cut is the first boundary c = k L, k >= 1, with T < fp32(eps) in front of it"""
    x = x_factors(sigma, t)
    R, S = x.shape
    L = segment_length(L, S)
    e = F32(eps)
    cut = np.full(R, S, dtype=np.int64)
    T = np.ones(R, dtype=F32)
    for i in range(S):
        if i > 0 and i % L == 0:
            cut[(cut == S) & (T < e)] = i
        T = (T * x[:, i]).astype(F32)
    return cut


def terminate(raw, t, eps, L, live=None):
    """raw [R, S, 4] of the dense pass -> (raw with the dead samples zeroed, cut [R], evaluated count).  live [R, S]: the grid's
    verdict (None: every sample occupied); the unoccupied samples are zeroed first, so they count as x = 1 in T"""
    raw = np.array(raw, dtype=F32, copy=True)
    R, S = raw.shape[:2]
    occ = np.ones((R, S), dtype=bool) if live is None else np.asarray(live, dtype=bool)
    raw[~occ] = 0
    cut = cuts(raw[..., 3], t, eps, L)
    before = np.arange(S)[None, :] < cut[:, None]
    raw[~before] = 0
    return raw, cut, int((occ & before).sum())


def boundary_transmittance(weights, L):
    """fp64 T in front of every segment boundary, from a render's weights [R, S]: 1 - sum_{i < c} w_i, for c = L, 2L, ... < S"""
    w = np.asarray(weights, dtype=np.float64)
    S = w.shape[1]
    L = segment_length(L, S)
    cs = np.arange(L, S, L)
    return cs, 1.0 - np.cumsum(w, axis=1)[:, cs - 1]
