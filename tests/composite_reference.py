"""NumPy references for csrc/composite.hip's training half (tests/test_composite_host.py proves what they are worth on the CPU,
tests/test_gpu_composite.py holds the kernel to them):

reference()  the yardstick.  The reference's float32 ELEMENTWISE semantics where they define the result (delta, exp, alpha and
             x = fl32(fl32(1 - alpha) + 1e-10): an opaque sample has x == 1e-10 exactly, as in TensorFlow), everything cumulative in
             float64 (exclusive product, sums, exclusive reverse sum Q, dalpha = dw T - Q / x, dsigma = dalpha delta ex, loss).  The
             clip gate is inclusive.  Fed float64 inputs it is float64 throughout (the tie to the oracle).
mirror32()   the same in float32 throughout in the KERNEL's structure: a lane-local run of C samples, six shuffle steps, butterfly
             sums, a true exclusive suffix sum (Ql + excls) -- not the oracle's `rev - prod`, which cancels to nothing on opaque rays
             and is then divided by 1e-10.
inputs()     ten ray classes interleaved by ray % 10.
MUTANTS      the reference with one mistake each.
"""
from __future__ import annotations

import functools

import numpy as np

F = np.float32
TOL_FACTOR = 8.0          # tol = 8 x the float32 mirror's error against the reference (the factor of tests/adam_reference.py)
POWER_FACTOR = 10.0       # every mutant is more than 10 x tol away
EDGE = 1e-5               # a ray is undecidable when a pre-clip channel lies this close to 0 or 1 without being on it
LAST_MIN = 1e-30          # the last sample's dsigma is compared relatively where |reference| is at least this (see last_mask)

R_CASE = 97               # not a multiple of 4: the last workgroup has three waves that leave early through the barrier path
# (250: the issue's list has no ragged run for composite_kernel<4>; 257 already takes <8>)
S_CASES = (2, 5, 33, 64, 65, 128, 130, 192, 250, 256, 257, 320, 512, 513, 768, 769, 1000, 1024)
CASES = [(S, white) for S in S_CASES for white in (0, 1)]
TILE_S = (32, 64, 192, 512, 1024)
LOSS0 = 0.75              # the loss is ADDED onto this

N_CLASSES = 10
ALL_ZERO, UNIFORM, LOG_RANGE, SPARSE_50, HALF_200, OPAQUE, RGB_OUTSIDE, OWN_PIXEL, UNSORTED, REPEATED_T = range(1, 11)

MUTANTS = ("last_delta_1e10", "inclusive_T", "strict_gate", "inclusive_suffix", "x_without_eps", "white_gsum_dropped",
           "no_lane_carry", "next_delta_in_dsigma", "grad_scale_on_clipped", "loss_scale_missing")


def template_C(S: int) -> int:
    """samples per lane of the composite_kernel<C> that launch_composite picks"""
    c = (S + 63) // 64
    return c if c <= 4 else (8 if c <= 8 else (12 if c <= 12 else 16))


def scales(R: int):
    """grad_scale, loss_scale of one chunk as knerf_train_chunk sets them"""
    return 2.0 / (3.0 * R), 1.0 / (3.0 * R)


# ---------------------------------------------------------------------------------------------------------------- inputs
def inputs(R: int, S: int, seed: int):
    """raw [R,S,4], t [R,S], target [R,3] float32 and cls [R] (1..10).  Rays of class OWN_PIXEL get their target from the caller: the
    ray's own rendered pixel (reference / mirror32: own_pixel=cls == OWN_PIXEL; on the device: knerf_composite's bits)."""
    rng = np.random.default_rng(seed)
    cls = (np.arange(R) % N_CLASSES) + 1
    t = (2.0 + 4.0 * (np.arange(S)[None, :] + rng.random((R, S))) / S).astype(F)
    t.sort(axis=-1)
    rgb = (0.02 + 0.96 * rng.random((R, S, 3))).astype(F)
    sigma = np.zeros((R, S), F)
    target = rng.random((R, 3)).astype(F)
    for r in range(R):
        c = cls[r]
        if c == UNIFORM:
            sigma[r] = 3.0 * rng.random(S)
        elif c == LOG_RANGE:
            sigma[r] = 10.0 ** rng.uniform(-6, 4, S)
        elif c == SPARSE_50:
            sigma[r] = np.where(rng.random(S) < 0.1, 50.0, 0.0)
        elif c == HALF_200:
            sigma[r] = np.where(rng.random(S) < 0.5, 0.0, 200.0 * rng.random(S))
        elif c == OPAQUE:
            sigma[r] = np.where(rng.random(S) < 0.1, 1e4, 0.0)
            sigma[r, min(S // 3, S - 2)] = 1e4               # a front in every ray, never on the last sample (delta 1e-10)
        elif c == RGB_OUTSIDE:
            # nearly opaque rays of one colour outside [0, 1]: pre = -0.5 or 1.5 on either background, the gate is closed in any arithmetic
            t[r] = (2.0 + 4.0 * (np.arange(S) + 0.25 + 0.5 * rng.random(S)) / S).astype(F)      # no tiny delta, also at S = 2
            sigma[r] = 50.0 + 50.0 * rng.random(S)
            rgb[r] = -0.5 if (r // N_CLASSES) % 2 == 0 else 1.5
        elif c == OWN_PIXEL:
            sigma[r] = 3.0 * rng.random(S)
        elif c == UNSORTED:
            # negative deltas, alpha < 0.  sigma ~ 2 / sum |delta|: |sigma delta| <= 3 on every sample and sum |w| stays of order 1, so
            # this class does not set the absolute tolerances of image, depth and weights for all the others
            t[r] = t[r][rng.permutation(S)]
            if (np.diff(t[r]) >= 0).all():
                t[r] = t[r][::-1].copy()
            sigma[r] = (0.5 + rng.random(S)) * 2.0 / max(np.abs(np.diff(t[r].astype(np.float64))).sum(), 1e-3)
        elif c == REPEATED_T:
            sigma[r] = 3.0 * rng.random(S)
            m = max(S // 2 - 1, 0)
            t[r, m + 1] = t[r, m]
    raw = np.concatenate([rgb, sigma[..., None]], axis=-1).astype(F)
    # Every target channel at least 0.05 away from the rendered pixel on either background: the whole draw of a ray scales with
    # df = image - target, and a ray that happens to hit its target to 1e-4 would set the relative tolerance of its whole case.
    imgs = [reference(raw, t, target, white, 1.0, 1.0)["image"] for white in (0, 1)]
    for _ in range(200):
        close = (np.abs(target - imgs[0]) < 0.05) | (np.abs(target - imgs[1]) < 0.05)
        if not close.any():
            break
        target[close] = rng.random(int(close.sum())).astype(F)
    assert not close.any()
    return dict(raw=np.ascontiguousarray(raw), t=np.ascontiguousarray(t), target=target, cls=cls)


# ------------------------------------------------------------------------------------------------------------- reference
def reference(raw, t, target, white, grad_scale, loss_scale, own_pixel=None, loss0=0.0, mutant=None):
    """dict(image, pre, depth, weights, draw, loss) in float64.  own_pixel: bool [R], rays whose target is their own image (df = 0)."""
    assert mutant is None or mutant in MUTANTS, mutant
    ft = raw.dtype.type                                   # float32: the elementwise semantics; float64: the oracle's arithmetic
    R, S = t.shape
    rgb, sigma = raw[..., :3].astype(np.float64), raw[..., 3]
    eps = ft(1e-10)
    last = ft(1e10) if mutant == "last_delta_1e10" else eps
    delta = np.concatenate([t[:, 1:] - t[:, :-1], np.full((R, 1), last, raw.dtype)], axis=-1)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        ex = np.exp(-(sigma * delta).astype(np.float64)).astype(raw.dtype)
        alpha = ft(1.0) - ex
        x = (ft(1.0) - alpha) if mutant == "x_without_eps" else ((ft(1.0) - alpha) + eps)
        delta, ex, alpha, x = (v.astype(np.float64) for v in (delta, ex, alpha, x))
        T = np.cumprod(x, axis=-1)
        if mutant != "inclusive_T":
            T = np.concatenate([np.ones((R, 1)), T[:, :-1]], axis=-1)
        w = alpha * T
        pre = np.sum(w[..., None] * rgb, axis=1)
        if white:
            pre = pre + (1.0 - np.sum(w, axis=-1))[:, None]
        image = np.clip(pre, 0.0, 1.0)
        depth = np.sum(w * t.astype(np.float64), axis=-1)
        tgt = target.astype(np.float64).copy()
        if own_pixel is not None:
            tgt[own_pixel] = image[own_pixel]
        df = image - tgt
        loss = loss0 + (1.0 if mutant == "loss_scale_missing" else loss_scale) * np.sum(df * df)
        gate = ((pre > 0.0) & (pre < 1.0)) if mutant == "strict_gate" else ((pre >= 0.0) & (pre <= 1.0))
        if mutant == "grad_scale_on_clipped":
            gate = np.ones_like(gate)
        g = np.where(gate, grad_scale * df, 0.0)
        dw = np.sum(rgb * g[:, None, :], axis=-1)
        if white and mutant != "white_gsum_dropped":
            dw = dw - np.sum(g, axis=-1)[:, None]
        prod = dw * w
        Q = np.zeros((R, S))                                   # true exclusive reverse sum: Q_k = sum_{i > k} prod_i
        if mutant == "no_lane_carry":                          # restarts at every lane's run of C samples
            C = (S + 63) // 64
            for k in range(S - 2, -1, -1):
                Q[:, k] = (Q[:, k + 1] + prod[:, k + 1]) if (k + 1) // C == k // C else 0.0
        else:
            Q[:, :-1] = np.cumsum(prod[:, :0:-1], axis=-1)[:, ::-1]
            if mutant == "inclusive_suffix":
                Q = Q + prod
        dalpha = dw * T - Q / x
        dl = np.concatenate([delta[:, 1:], delta[:, -1:]], axis=-1) if mutant == "next_delta_in_dsigma" else delta
        dsigma = dalpha * dl * ex
        draw = np.concatenate([w[..., None] * g[:, None, :], dsigma[..., None]], axis=-1)
    return dict(image=image, pre=pre, depth=depth, weights=w, draw=draw, loss=float(loss))


# ---------------------------------------------------------------------------------------------------------------- mirror
def exp_numpy(a):
    return np.exp(a)


def exp_jittered(seed):
    """NumPy's float32 exp with every result moved one ulp up or down at random (the device's expf is not NumPy's).  Results that are exactly
    1 (an argument below half an ulp of 1, zero included: any expf returns 1 there), 0 or inf stay what they are."""
    rng = np.random.default_rng(seed)

    def f(a):
        with np.errstate(over="ignore"):
            e = np.exp(a)
        up = rng.random(a.shape) < 0.5
        j = np.nextafter(e, np.where(up, F(np.inf), F(0.0)).astype(F))
        keep = (e == 1) | (e == 0) | ~np.isfinite(e)
        return np.where(keep, e, j).astype(F)
    return f


def _wave_sum(v):
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def mirror32(raw, t, target, white, grad_scale, loss_scale, own_pixel=None, exp=exp_numpy):
    """composite_kernel<C> in float32 NumPy, operation by operation (no fused multiply-add: the library is built with
    -ffp-contract=off).  Returns dict(image, pre, depth, weights, draw, partial): partial [ceil(R/4)] the workgroups' loss terms."""
    assert raw.dtype == F and t.dtype == F and target.dtype == F
    R, S = t.shape
    C = template_C(S)
    P = 64 * C
    one, zero, eps = F(1.0), F(0.0), F(1e-10)
    gs, ls = F(grad_scale), F(loss_scale)

    def lanes(a, fill):
        out = np.full((R, P), fill, F)
        out[:, :S] = a
        return out.reshape(R, 64, C)
    ok = lanes(np.ones((R, S), F), 0.0) > 0
    r, g, b, sg = (lanes(raw[..., k], 0.0) for k in range(4))
    tt = lanes(t, 0.0)
    tn = np.zeros((R, S), F)
    tn[:, :-1] = t[:, 1:]
    dl = lanes(tn - t, 0.0)
    dl.reshape(R, P)[:, S - 1:] = eps                       # i + 1 >= S
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        ex = exp(-(sg * dl)).astype(F)
        al = np.where(ok, one - ex, zero)
        x = np.where(ok, (one - al) + eps, one)
        T = np.empty((R, 64, C), F)
        run = np.ones((R, 64), F)
        for c in range(C):
            T[:, :, c] = run
            run = run * x[:, :, c]
        inc = run
        for o in (1, 2, 4, 8, 16, 32):
            new = inc.copy()
            new[:, o:] = inc[:, o:] * inc[:, :-o]
            inc = new
        excl = np.ones((R, 64), F)
        excl[:, 1:] = inc[:, :-1]
        acc = [np.zeros((R, 64), F) for _ in range(5)]
        w = np.empty((R, 64, C), F)
        for c in range(C):
            T[:, :, c] = T[:, :, c] * excl
            w[:, :, c] = al[:, :, c] * T[:, :, c]
            for k, v in enumerate((r, g, b, tt)):
                acc[k] = acc[k] + w[:, :, c] * v[:, :, c]
            acc[4] = acc[4] + w[:, :, c]
        sr, sgc, sb, sd, sw = (_wave_sum(v) for v in acc)
        pre = np.stack([sr, sgc, sb], axis=-1)
        if white:
            pre = pre + (one - sw)[:, None]
        img = np.minimum(np.maximum(pre, zero), one)
        tgt = target.copy()
        if own_pixel is not None:
            tgt[own_pixel] = img[own_pixel]
        df = img - tgt
        l2 = ((zero + df[:, 0] * df[:, 0]) + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]
        gi = np.where((pre >= zero) & (pre <= one), gs * df, zero).astype(F)
        sl = np.zeros(((R + 3) // 4) * 4, F)
        sl[:R] = l2 * ls
        sl = sl.reshape(-1, 4)
        partial = (sl[:, 0] + sl[:, 1]) + (sl[:, 2] + sl[:, 3])
        gsum = ((gi[:, 0] + gi[:, 1]) + gi[:, 2]) if white else np.zeros(R, F)
        g0, g1, g2, gsum = (v[:, None] for v in (gi[:, 0], gi[:, 1], gi[:, 2], gsum))
        dw = np.empty((R, 64, C), F)
        Ql = np.empty((R, 64, C), F)
        suffix = np.zeros((R, 64), F)
        for c in range(C - 1, -1, -1):
            dw[:, :, c] = ((g0 * r[:, :, c] + g1 * g[:, :, c]) + g2 * b[:, :, c]) - gsum
            Ql[:, :, c] = suffix
            suffix = suffix + dw[:, :, c] * w[:, :, c]
        incs = suffix
        for o in (1, 2, 4, 8, 16, 32):
            new = incs.copy()
            new[:, :-o] = incs[:, :-o] + incs[:, o:]
            incs = new
        excls = np.zeros((R, 64), F)
        excls[:, :-1] = incs[:, 1:]
        Q = Ql + excls[:, :, None]
        dalpha = dw * T - Q / x
        dsig = (dalpha * dl) * ex
        draw = np.stack([w * g0[:, :, None], w * g1[:, :, None], w * g2[:, :, None], dsig], axis=-1)
    flat = lambda a: a.reshape(R, P, *a.shape[3:])[:, :S]
    return dict(image=img, pre=pre, depth=sd, weights=flat(w), draw=flat(draw).astype(F), partial=partial.astype(F))


def atomic_loss32(partial, loss0):
    """the default mode's loss: one float32 atomic per workgroup, here in workgroup order"""
    s = F(loss0)
    for p in partial:
        s = F(s + p)
    return float(s)


# ------------------------------------------------------------------------------------------- errors, the cap, tolerances
def undecidable(ref):
    """rays whose clip gate float32 and float64 may decide differently: some pre-clip channel of the float64 reference within EDGE of 0
    or 1 without being exactly on it"""
    p = ref["pre"]
    near = ((np.abs(p) < EDGE) & (p != 0.0)) | ((np.abs(p - 1.0) < EDGE) & (p != 1.0))
    return near.any(axis=-1)


def last_mask(ref, skip):
    """rays whose last sample's dsigma is compared relative to its own reference value: decidable, and large enough for the float32
    product dw T 1e-10 ex to stay a normal number (behind an opaque front T underflows and there is nothing relative to compare)"""
    return ~skip & (np.abs(ref["draw"][:, -1, 3]) >= LAST_MIN)


def draw_error(draw, ref_draw):
    """per ray: max |draw - ref| as a share of that ray's max |ref|; a ray whose reference is all zero must be all zero (else inf)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.asarray(draw, np.float64) - ref_draw).reshape(len(ref_draw), -1)
        d = np.where(np.isfinite(d), d, np.inf).max(axis=1)
    scale = np.abs(ref_draw).reshape(len(ref_draw), -1).max(axis=1)
    zero_ok = (np.asarray(draw).reshape(len(ref_draw), -1) == 0).all(axis=1)
    return np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(zero_ok, 0.0, np.inf))


def errors(out, ref, skip):
    """the checked figures of `out` (image, depth, weights, draw and optionally loss) against the reference; `skip`: the undecidable
    rays, left out of the gated comparisons (draw and the last sample's dsigma)"""
    def mx(a):
        a = np.abs(np.asarray(a, np.float64))
        return float(np.where(np.isfinite(a), a, np.inf).max()) if a.size else 0.0
    e = dict(image=mx(out["image"] - ref["image"]), depth=mx(out["depth"] - ref["depth"]), weights=mx(out["weights"] - ref["weights"]))
    e["draw"] = float(draw_error(out["draw"], ref["draw"])[~skip].max())
    m = last_mask(ref, skip)
    rl = ref["draw"][m, -1, 3]
    e["last"] = mx((np.asarray(out["draw"], np.float64)[m, -1, 3] - rl) / rl)
    if "loss" in out:
        e["loss"] = mx(out["loss"] - ref["loss"])
    return e


def loss_mirror_error(partial32, ref_partial64, loss0):
    """The loss is ONE number: the signed error of one float32 evaluation can cancel to nothing by chance, and the device adds the
    workgroups' terms in no fixed order.  The figure used instead is what bounds the mirror's error under ANY order: the sum of the
    magnitudes of the errors of the workgroups' terms, plus half an ulp of the largest running sum for every addition."""
    n = len(partial32)
    top = abs(loss0) + float(np.abs(ref_partial64).sum())
    return float(np.abs(partial32.astype(np.float64) - ref_partial64).sum()) + (n + 1) * 2.0 ** -24 * top


def ref_partials(ref_image, target, own_pixel, loss_scale):
    """the workgroups' loss terms of the float64 reference (four rays each)"""
    tgt = target.astype(np.float64).copy()
    tgt[own_pixel] = ref_image[own_pixel]
    l2 = ((ref_image - tgt) ** 2).sum(axis=1) * loss_scale
    l2 = np.concatenate([l2, np.zeros(-len(l2) % 4)])
    return l2.reshape(-1, 4).sum(axis=1)


@functools.lru_cache(maxsize=None)
def case(S: int, white: int, R: int = R_CASE):
    """inputs, reference, undecidable rays and tolerances of one case; computed once, shared by every test, never modified"""
    I = inputs(R, S, seed=1000 * S + white)
    gs, ls = scales(R)
    own = I["cls"] == OWN_PIXEL
    ref = reference(I["raw"], I["t"], I["target"], white, gs, ls, own_pixel=own, loss0=LOSS0)
    skip = undecidable(ref)
    rp = ref_partials(ref["image"], I["target"], own, ls)
    err = {}
    for name, fn in (("numpy", exp_numpy), ("jitter", exp_jittered(7 + S))):
        m = mirror32(I["raw"], I["t"], I["target"], white, gs, ls, own_pixel=own, exp=fn)
        e = errors(m, ref, skip)
        e["loss"] = loss_mirror_error(m["partial"], rp, LOSS0)
        err[name] = e
    mirror = {k: max(err["numpy"][k], err["jitter"][k]) for k in err["numpy"]}
    tol = {k: TOL_FACTOR * v for k, v in mirror.items()}
    for a in list(I.values()) + [v for v in ref.values() if isinstance(v, np.ndarray)] + [skip]:
        a.setflags(write=False)
    return dict(I, own=own, grad_scale=gs, loss_scale=ls, ref=ref, skip=skip, mirror_err=mirror, mirror_errs=err, tol=tol)


# ----------------------------------------------------------------------------------------------------------- tile outputs
def dead_tiles(draw, raw):
    """composite.hip's dead rule from a draw and its raw: a sample is dead when drgb == 0 and (dsigma == 0 or sigma == 0); a 32-sample
    tile is dead when all its samples are.  Returns live flags [R * S/32] int32 (1 = live), the layout of tile_flags."""
    R, S = draw.shape[:2]
    dead = (draw[..., 0] == 0) & (draw[..., 1] == 0) & (draw[..., 2] == 0) & ((draw[..., 3] == 0) | (raw[..., 3] == 0))
    return (~dead).reshape(R, S // 32, 32).any(axis=-1).astype(np.int32).reshape(-1)


def compact_reference(flags, period, real):
    """compact_tiles_kernel: ascending indices i with flags[i] != 0 and (i % period) < real; the number of real tiles"""
    i = np.arange(len(flags))
    is_real = (i % period) < real
    return i[(flags != 0) & is_real].astype(np.int32), int(is_real.sum())
