"""The sampler's untested branches (csrc/sampler.hip sample_fine_kernel, csrc/utils_ops.hip inverse_cdf_kernel), bit for bit against
oracle.fine_points / oracle.fine_hierarchical_sampling_chunk in both out-of-range modes, with injected weights and u:

* u exactly on every knot of oracle.cdf_from_weights(w), one ulp to either side of each, u = 0, u = 1 - 2^-24, and u >= cdf[-1]
  where rounding leaves cdf[-1] < 1 (searchsorted returns Nc + 1: both gathers are past the end of the mid-points);
* all-zero weights; one weight of 1e6 among zeros (the `denom < 1e-5` branch on almost every bin); peaky and flat weights;
* sorted, repeated and UNSORTED coarse t -- the last takes the `!sorted` ranking fallback of sample_fine_kernel's merge;
* Nc in {2, 3, 64, 65, 512} x Nf in {1, 3, 64, 65, 512}: below, on and above a wavefront's 64 lanes, and the limits.

Every (weights, t) combination gets as many rays as it takes to place each u of its pool once; all rays of a shape go through
one launch."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

F = np.float32
U_MAX = F(1.0 - 2.0 ** -24)
NC = (2, 3, 64, 65, 512)
NF = (1, 3, 64, 65, 512)


def coarse_weights(Nc, rng):
    one_big = np.zeros(Nc, F)
    one_big[Nc // 3] = 1e6
    for seed in range(1000):                                     # random weights whose cdf ends BELOW 1 in float32
        short = np.random.default_rng(seed).random(Nc).astype(F)
        if O.cdf_from_weights(short[None])[0, -1] < 1:
            break
    return {"peaky": (rng.random(Nc) ** 8).astype(F), "zero": np.zeros(Nc, F), "one_1e6": one_big, "flat": np.ones(Nc, F), "short": short}


def coarse_t(Nc, rng):
    t = np.sort((2.0 + 4.0 * (np.arange(Nc) + rng.random(Nc)) / Nc).astype(F))
    rep = t.copy()
    rep[1::3] = rep[0:-1:3][:len(rep[1::3])]                     # every third value repeats its predecessor
    uns = t[rng.permutation(Nc)]
    if (np.diff(uns) >= 0).all():
        uns = uns[::-1].copy()
    return {"sorted": t, "repeated": rep, "unsorted": uns}


def u_pool(w, rng):
    cdf = O.cdf_from_weights(w[None])[0]
    pool = np.concatenate([cdf, np.nextafter(cdf, F(-1)), np.nextafter(cdf, F(2)), [F(0), U_MAX], rng.random(8, dtype=F)]).astype(F)
    return np.unique(pool[(pool >= 0) & (pool <= U_MAX)]), cdf


@pytest.fixture(scope="module")
def problems():
    out = {}
    for Nc in NC:
        rng = np.random.default_rng(Nc)
        W, T = coarse_weights(Nc, rng), coarse_t(Nc, rng)
        pools = {k: u_pool(w, rng) for k, w in W.items()}
        out[Nc] = (W, T, pools)
    return out


def build(problems, Nc, Nf):
    W, T, pools = problems[Nc]
    rng = np.random.default_rng(1000 * Nc + Nf)
    ts, ws, us = [], [], []
    for wk, w in W.items():
        pool, _ = pools[wk]
        for tk, t in T.items():
            n = -(-len(pool) // Nf)
            u = np.concatenate([rng.permutation(pool), rng.random(n * Nf - len(pool), dtype=F)]).reshape(n, Nf)
            ts.append(np.tile(t, (n, 1))); ws.append(np.tile(w, (n, 1))); us.append(u)
    return np.concatenate(ts), np.concatenate(ws), np.concatenate(us).astype(F)


def test_the_pools_hold_the_edges(problems):
    """what the u values promise (no GPU needed)"""
    for Nc, (W, T, pools) in problems.items():
        for wk, (pool, cdf) in pools.items():
            assert np.isin(cdf[cdf <= U_MAX], pool).all() and F(0) in pool and U_MAX in pool
            assert pool.min() >= 0 and pool.max() < 1
            if wk == "one_1e6" and Nc > 2:
                assert (np.diff(cdf) < 1e-5).sum() >= Nc - 1                  # the denom branch on every bin but one
        cdf = pools["short"][1]
        assert cdf[-1] < 1 and (pools["short"][0] >= cdf[-1]).any()           # rounding leaves cdf[-1] < 1, with u at (and above) it
        assert (np.diff(T["unsorted"]) < 0).any() and (np.diff(T["repeated"]) == 0).any() == (Nc >= 2)


@pytest.mark.gpu
@pytest.mark.parametrize("Nf", NF)
@pytest.mark.parametrize("Nc", NC)
def test_sampler_edges_bit_exact(problems, Nc, Nf):
    from keras_nerf_amd import _lib
    from keras_nerf_amd.runtime import KnerfContext, _ptr
    t, w, u = build(problems, Nc, Nf)
    R = len(t)
    mids = np.ascontiguousarray(F(0.5) * (t[:, 1:] + t[:, :-1])) if Nc > 1 else None
    dt, dw, du, dm = (torch.from_numpy(a).cuda() for a in (t, w, u, mids))
    lib = _lib.load()
    differ = False
    for oob in ("zero", "clamp"):
        ctx = KnerfContext(n_coarse=Nc, n_fine=Nf, oob=oob)
        got = ctx.sample_fine(dt, dw, du).cpu().numpy()
        fine = torch.empty((R, Nf), device="cuda")
        assert lib.knerf_inverse_cdf(ctx._stream(), _ptr(dm), _ptr(dw), _ptr(du), R, Nc - 1, Nc, Nf, int(oob == "clamp"), _ptr(fine)) == 0
        fine = fine.cpu().numpy()
        ctx.close()
        want_fine = O.fine_hierarchical_sampling_chunk(mids, w, u, oob)
        want = O.fine_points(t, w, u, oob)
        assert np.isfinite(want).all()
        np.testing.assert_array_equal(fine, want_fine)
        np.testing.assert_array_equal(got, want)
        assert (np.diff(got, axis=1) >= 0).all()
        differ = differ or oob == "clamp" and not np.array_equal(want, O.fine_points(t, w, u, "zero"))
    assert differ                                  # the out-of-range gathers are really taken: the two modes give different values
