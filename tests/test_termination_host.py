"""Early ray termination's host side, no GPU needed: the NumPy cut-rule mirror (tests/termination_reference.py) on hand-made sigma / t
cases -- an opaque slab, rays that never reach eps, a sample count that is not a multiple of L, L = 1 -- the bounds on the image and
depth that the cut implies, and argument validation of NeRF.set_ray_termination."""
import numpy as np
import pytest

from oracle import nerf_oracle as O
from tests import termination_reference as M


def _t(R, S, near=2.0, far=6.0):
    return np.tile(np.linspace(near, far, S, dtype=np.float32), (R, 1))


def test_opaque_slab_cuts_at_the_next_boundary():
    R, S, L = 3, 40, 8
    t = _t(R, S)
    sigma = np.zeros((R, S), np.float32)
    sigma[0, 10:15] = 1e3                   # ray 0: opaque from sample 10: T < eps in front of sample 11, next boundary 16
    sigma[1, 16:20] = 1e3                   # ray 1: opaque from 16 exactly: T drops behind it, cut at 24
    sigma[2, 3] = 1e3                       # ray 2: inside segment 0: cut at 8
    cut = M.cuts(sigma, t, 1e-4, L)
    assert cut.tolist() == [16, 24, 8]
    # T in front of the cut, from the fp32 weights, is below eps; in front of the boundary before it, above
    _, _, w = O.render_image_depth_chunk(np.zeros((R, S, 3), np.float32), sigma, t, False)
    for r, c in enumerate(cut):
        cs, T = M.boundary_transmittance(w[r:r + 1], L)
        k = list(cs).index(c)
        assert T[0, k] < 1e-4 and (k == 0 or T[0, k - 1] >= 1e-4)


def test_never_reaching_eps_cuts_nothing():
    R, S = 4, 64
    rng = np.random.default_rng(0)
    sigma = rng.uniform(0, 0.5, (R, S)).astype(np.float32)
    assert (M.cuts(sigma, _t(R, S), 1e-4, 16) == S).all()
    assert (M.cuts(np.full((R, S), 1e3, np.float32), _t(R, S), 0.0, 16) == S).all()      # eps = 0: T < 0 never holds


def test_samples_not_a_multiple_of_the_segment():
    R, S, L = 2, 10, 4                      # segments [0, 4), [4, 8), [8, 10)
    t = _t(R, S)
    sigma = np.zeros((R, S), np.float32)
    sigma[0, 5] = 1e3                       # cut at 8: the short last segment goes
    sigma[1, 9] = 1e3                       # the last sample's opacity ends nothing: no boundary behind it
    assert M.cuts(sigma, t, 1e-3, L).tolist() == [8, 10]
    assert M.cuts(sigma, t, 1e-3, 64).tolist() == [10, 10]       # L > S: one segment, nothing is ever cut


def test_segment_of_one_sample():
    R, S = 2, 12
    t = _t(R, S)
    sigma = np.zeros((R, S), np.float32)
    sigma[0, 4] = 1e3
    sigma[1, 2:] = 2.0                      # a gradual decay: the cut is the first sample whose T is below eps
    cut = M.cuts(sigma, t, 1e-2, 1)
    assert cut[0] == 5
    x = M.x_factors(sigma, t)[1]
    T = np.cumprod(np.concatenate([[1.0], x[:-1]]).astype(np.float32), dtype=np.float32)
    assert cut[1] == int(np.argmax(T < np.float32(1e-2)))
    assert T[cut[1] - 1] >= np.float32(1e-2)


def test_the_cut_moves_image_and_depth_within_eps():
    rng = np.random.default_rng(1)
    R, S, L, eps = 256, 96, 16, 1e-3
    t = np.sort(rng.uniform(2, 6, (R, S)), axis=1).astype(np.float32)
    raw = np.concatenate([rng.random((R, S, 3)), rng.exponential(60.0, (R, S, 1)) * (rng.random((R, S, 1)) < 0.3)], -1).astype(np.float32)
    live = rng.random((R, S)) < 0.8
    dense = raw.copy(); dense[~live] = 0
    cut_raw, cut, n_eval = M.terminate(raw, t, eps, L, live)
    assert (cut < S).mean() > 0.2 and n_eval == int((live & (np.arange(S) < cut[:, None])).sum())
    for white in (False, True):
        i0, d0, w0 = O.render_image_depth_chunk(dense[..., :3], dense[..., 3], t, white)
        i1, d1, w1 = O.render_image_depth_chunk(cut_raw[..., :3], cut_raw[..., 3], t, white)
        before = np.arange(S)[None, :] < cut[:, None]
        assert np.array_equal(w1[before], w0[before]) and (w1[~before] == 0).all()
        assert np.abs(i1 - i0).max() <= eps + 1e-6
        assert np.abs(d1 - d0).max() <= eps * 6.0 + 1e-5


@pytest.mark.parametrize("bad", [dict(threshold=-1e-3), dict(threshold=1.0), dict(threshold=float("nan")), dict(threshold=float("inf")),
                                 dict(threshold=True), dict(threshold="1e-4"), dict(threshold=None), dict(segment=0),
                                 dict(segment=1025), dict(segment=32.0), dict(segment=True), dict(segment="32")])
def test_set_ray_termination_rejects_bad_arguments(bad):
    from keras_nerf_amd.model.nerf.nerf import NeRF
    with pytest.raises(ValueError):
        NeRF().set_ray_termination(**bad)


def test_set_ray_termination_needs_a_compiled_model():
    from keras_nerf_amd.model.nerf.nerf import NeRF
    with pytest.raises(RuntimeError):
        NeRF().set_ray_termination(1e-4)
    with pytest.raises(RuntimeError):
        NeRF().termination_stats()


def test_the_header_documents_the_options():
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "knerf.h")).read()
    for name in ('"termination_threshold"', '"termination_segment"', "knerf_termination_stats"):
        assert name in h, name
