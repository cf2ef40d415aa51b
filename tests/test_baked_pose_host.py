"""Refining camera poses against a baked field, the parts that need no device: the fp64 reference of the ray gradients
(tests/baked_pose_reference.py) against central differences of its own loss, the reduction to cameras against central differences
under R <- exp(eps^) R, t <- t + tau, Rodrigues, the pose update with fixed views, the argument checks with the NDC refusal, and the
additive hook of RayBatchDataset.  tests/README_baked_pose.md has the convergence record of the differences.

The loss is piecewise smooth: its derivative jumps where a sample changes its cell and where a clamp starts to act.  So the tests take
only rays whose samples keep CELL_MARGIN = 1e-3 cell from every cell boundary and CLAMP_MARGIN = 1e-3 from both clamps (asserted on the
reference's own per-ray margins), termination 0, and move a ray by H = 2e-6: at most 2e-6 x 6.5 x 4.6 = 6e-5 cell, far inside the
margin, so no difference straddles a jump.  Tolerance: central differences have an error c H^2; halving the step shows it:
|D(2H) - D(H)| = 3 c H^2 bounds D(H)'s own error c H^2 three times over, and the rounding of the two losses adds about
2^-52 L / H = 1e-11.  So |D(H) - g| <= |D(2H) - D(H)| + 1e-9 max |g| is asserted, element by element: a bound from the loss alone.
"""
import numpy as np
import pytest

from tests import baked_pose_reference as P
from tests import baked_train_reference as T

RES = (9, 8, 7)
LO, HI = (-1.0, -0.8, -0.6), (1.0, 0.8, 0.7)
STEP = 0.08
CELL_MARGIN, CLAMP_MARGIN, H = 1e-3, 1e-3, 2e-6


def _lattice(degree, seed=3):
    rng = np.random.default_rng(seed + degree)
    sigma = rng.uniform(0.0, 3.0, RES).astype(np.float32)
    sigma[0], sigma[-1], sigma[:, 0], sigma[:, -1], sigma[:, :, 0], sigma[:, :, -1] = 0, 0, 0, 0, 0, 0     # no jump at the box face
    sigma[3:5, 2:4, 2:4] = 0                                                                              # a cell outside the support
    K = (degree + 1) ** 2
    co = (rng.standard_normal(RES + (K, 3)) * 0.05).astype(np.float16)
    co[..., 0, :] += np.float16(1.5)
    return sigma, co.astype(np.float64)


def _smooth_rays(sigma, co, white, n_keep, seed, origins=None, directions=None):
    """candidate rays towards the box, those kept whose margins hold: (o, d, near, far, target) in float64 / float32"""
    rng = np.random.default_rng(seed)
    n = 60
    if origins is None:
        o = rng.standard_normal((n, 3)); o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
        d = rng.uniform(-0.4, 0.4, (n, 3)) - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[::3] *= rng.uniform(0.3, 3.0, (len(d[::3]), 1))                  # every third direction is no unit vector
    else:
        o, d = origins, directions
        n = o.shape[0]
    near = np.zeros(n, dtype=np.float32)
    far = (6.0 / np.linalg.norm(d, axis=1)).astype(np.float32)
    target = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    info = {}
    P.ray_gradients(sigma, co, LO, HI, o, d, near, far, STEP, target, T.support_cells(sigma), white, info=info, rays64=True)
    ok = np.nonzero((info["cell_margin"] >= CELL_MARGIN) & (info["clamp_margin"] >= CLAMP_MARGIN) & (info["opacity"] > 0.05))[0][:n_keep]
    return ok, (o, d, near, far, target)


def _loss(sigma, co, white, o, d, near, far, target, n_norm):
    return P.ray_gradients(sigma, co, LO, HI, o, d, near, far, STEP, target, T.support_cells(sigma), white, n_norm=n_norm, rays64=True)[0]


@pytest.mark.parametrize("degree,white", [(0, False), (1, True), (2, False), (3, True)])
def test_ray_gradients_are_the_derivative_of_the_loss(degree, white):
    sigma, co = _lattice(degree)
    ok, (o, d, near, far, target) = _smooth_rays(sigma, co, white, 5, 40 + degree)
    assert len(ok) == 5 and (np.abs(np.linalg.norm(d[ok], axis=1) - 1) > 0.05).any()             # a non-unit direction is among them
    o, d, near, far, target = (x[ok] for x in (o, d, near, far, target))
    info = {}
    N = len(ok)
    _, go, gd = P.ray_gradients(sigma, co, LO, HI, o, d, near, far, STEP, target, T.support_cells(sigma), white, info=info, rays64=True)
    assert info["cell_margin"].min() >= CELL_MARGIN and info["clamp_margin"].min() >= CLAMP_MARGIN      # checked by the test itself
    worst = (0.0, 0.0, 0.0)
    for r in range(N):
        one = lambda oo, dd: _loss(sigma, co, white, oo[None], dd[None], near[r:r + 1], far[r:r + 1], target[r:r + 1], N)
        for which, g in (("o", go), ("d", gd)):
            for a in range(3):
                D = []
                for h in (2 * H, H):
                    e = np.zeros(3); e[a] = h
                    D.append((one(o[r] + e, d[r]) - one(o[r] - e, d[r])) / (2 * h) if which == "o" else
                             (one(o[r], d[r] + e) - one(o[r], d[r] - e)) / (2 * h))
                tol = abs(D[0] - D[1]) + 1e-9 * max(np.abs(go).max(), np.abs(gd).max())
                err = abs(D[1] - g[r, a])
                assert err <= tol, (degree, r, which, a, err, tol)
                worst = max(worst, (err, abs(D[0] - D[1]), abs(g[r, a])))
    print(f"degree {degree} white {white}: largest |D(H) - g| {worst[0]:.3e} where |D(2H) - D(H)| = {worst[1]:.3e} and |g| = {worst[2]:.3e}; "
          f"max |grad_origin| {np.abs(go).max():.3e}, max |grad_direction| {np.abs(gd).max():.3e}")
    assert np.abs(go).max() > 1e-3 and np.abs(gd).max() > 1e-3


def test_zero_direction_and_missing_rays_have_no_gradient():
    sigma, co = _lattice(1)
    o = np.array([[0.1, 0.1, 0.1], [3.0, 3.0, 3.0]]); d = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    L, go, gd = P.ray_gradients(sigma, co, LO, HI, o, d, 0.0, 6.0, STEP, np.full((2, 3), 0.5), T.support_cells(sigma))
    assert (go == 0).all() and (gd == 0).all() and np.isfinite(L)


def _cameras(rng, V):
    c2w = np.tile(np.eye(4), (V, 1, 1))
    for v in range(V):
        eye = rng.standard_normal(3); eye = 3.0 * eye / np.linalg.norm(eye)
        fwd = -eye / 3.0
        right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
        c2w[v, :3, 0], c2w[v, :3, 1], c2w[v, :3, 2], c2w[v, :3, 3] = right, np.cross(right, fwd), -fwd, eye
    return c2w


@pytest.mark.parametrize("normalised", [False, True])
def test_pose_gradients_are_the_derivative_under_a_rigid_motion(normalised):
    """rays o = t, d = R cam (or R cam / |R cam|) of 3 cameras; the loss differenced under R <- exp(eps e_a ^) R and t <- t + eps e_a"""
    degree, white, V = 2, False, 3
    sigma, co = _lattice(degree)
    rng = np.random.default_rng(8)
    c2w = _cameras(rng, V)
    cam = np.concatenate([rng.uniform(-0.12, 0.12, (20, 2)), -np.ones((20, 1))], axis=1)
    view_all = np.repeat(np.arange(V), 20)

    def rays(poses, keep=slice(None)):
        d = np.einsum("vab,pb->vpa", poses[:, :3, :3], cam).reshape(-1, 3)
        if normalised:
            d = d / np.linalg.norm(d, axis=1, keepdims=True)
        o = np.repeat(poses[:, :3, 3], 20, axis=0)
        return o[keep], d[keep]
    o, d = rays(c2w)
    ok, (_, _, near, far, target) = _smooth_rays(sigma, co, white, 60, 9, o, d)
    view = view_all[ok]
    assert all((view == v).sum() >= 3 for v in range(V)), np.bincount(view)
    # near / far are held fixed as the cameras move (the discontinuities carry no gradient)
    near, far, target = near[ok], far[ok], target[ok]
    N = len(ok)
    o, d = rays(c2w, ok)
    _, go, gd = P.ray_gradients(sigma, co, LO, HI, o, d, near, far, STEP, target, T.support_cells(sigma), white, rays64=True)
    G = P.pose_gradients(go, gd, d, view, V + 1)
    assert (G[V] == 0).all() and np.abs(G[:V]).min() > 0                   # a view without a ray gets zeros
    worst = 0.0
    for v in range(V):
        for a in range(6):
            D = []
            for h in (2 * H, H):
                L = []
                for s in (1.0, -1.0):
                    motion = np.zeros((V, 6)); motion[v, a] = s * h
                    oo, dd = rays(P.move_poses(c2w, motion[:, 3:], motion[:, :3]), ok)
                    L.append(_loss(sigma, co, white, oo, dd, near, far, target, N))
                D.append((L[0] - L[1]) / (2 * h))
            tol = abs(D[0] - D[1]) + 1e-9 * np.abs(G).max()
            assert abs(D[1] - G[v, a]) <= tol, (v, a, D[1], G[v, a], tol)
            worst = max(worst, abs(D[1] - G[v, a]))
    print(f"normalised {normalised}: largest |D(H) - G| {worst:.3e}, max |G| {np.abs(G).max():.3e}")


def test_pose_gradients_skip_what_is_out_of_range():
    rng = np.random.default_rng(2)
    go, gd, d = (rng.standard_normal((50, 3)) for _ in range(3))
    view = rng.integers(0, 4, 50)
    ref = P.pose_gradients(go, gd, d, view, 4)
    view2 = np.concatenate([view, [-1, 4, 99]])
    ext = lambda x: np.concatenate([x, np.ones((3, 3))])
    assert np.array_equal(P.pose_gradients(ext(go), ext(gd), ext(d), view2, 4), ref)
    assert np.allclose(ref[2, 3:], np.cross(d[view == 2], gd[view == 2]).sum(axis=0))


def test_rodrigues():
    import torch
    from keras_nerf_amd.baked_pose import rodrigues
    rng = np.random.default_rng(0)
    w = np.concatenate([np.zeros((1, 3)), rng.standard_normal((20, 3)) * 1e-7, rng.standard_normal((20, 3)) * 1e-4,
                        rng.standard_normal((20, 3)) * 0.03, rng.standard_normal((20, 3)) * 2.0])
    for R in (P.rodrigues(w), rodrigues(torch.as_tensor(w)).numpy()):
        assert np.array_equal(R[0], np.eye(3))                              # at zero it is the identity
        assert np.abs(R @ np.transpose(R, (0, 2, 1)) - np.eye(3)).max() <= 1e-12
        assert np.abs(np.linalg.det(R) - 1).max() <= 1e-12
        assert np.abs(np.einsum("vab,vb->va", R, w) - w).max() <= 1e-12      # the axis stays
    # two libraries' sin and cos may differ by an ulp, and K K has entries up to |omega|^2 = 40 here
    assert np.abs(P.rodrigues(w) - rodrigues(torch.as_tensor(w)).numpy()).max() <= 1e-13
    quarter = P.rodrigues(np.array([0.0, 0.0, np.pi / 2]))
    assert np.abs(quarter @ np.array([1.0, 0.0, 0.0]) - np.array([0.0, 1.0, 0.0])).max() <= 1e-15
    assert np.abs(P.rodrigues(w[50]) @ P.rodrigues(-w[50]) - np.eye(3)).max() <= 1e-12


def test_pose_update_and_fixed_views():
    """PoseOptimizer.apply on host tensors against pose_adam_step, three steps; fixed views keep pose and moments bit for bit"""
    import torch
    from keras_nerf_amd.baked_pose import PoseOptimizer, fixed_mask, pose_errors
    rng = np.random.default_rng(4)
    V = 6
    c2w = _cameras(rng, V).astype(np.float32)
    hyper = dict(learning_rate_rotation=3e-3, learning_rate_translation=2e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
    for fixed in ([1, 4], np.array([False, True, False, False, True, False]), torch.as_tensor([1, 4])):
        po = PoseOptimizer(c2w, fixed_views=fixed, device="cpu", **hyper)
        assert np.array_equal(po.poses.numpy().view(np.uint32), c2w.view(np.uint32)) and po.poses.dtype == torch.float32
        assert po.fixed_views.tolist() == [False, True, False, False, True, False]
        live = po.poses
        want, m, v = c2w.astype(np.float64), np.zeros((V, 6)), np.zeros((V, 6))
        for t in (1, 2, 3):
            g = rng.standard_normal((V, 6)) * 1e-3
            po._grad += torch.as_tensor(g)
            assert np.array_equal(po.gradients().numpy(), g)
            start = po.poses.numpy().astype(np.float64)
            want, m, v = P.pose_adam_step(start, m, v, g, 3e-3, 2e-3, 0.9, 0.999, 1e-7, t, fixed=po.fixed_views.numpy())
            po.apply()
            got = po.poses.numpy()
            assert po.step == t and po.poses is live and float(po.gradients().abs().max()) == 0.0
            assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 1e-14).all()
            assert np.abs(po._m.numpy() - m).max() <= 1e-15 and np.abs(po._v.numpy() - v).max() <= 1e-15
            for f in (1, 4):
                assert np.array_equal(got[f].view(np.uint32), c2w[f].view(np.uint32))
                assert (po._m.numpy()[f] == 0).all() and (po._v.numpy()[f] == 0).all()
            # Adam's first step moves every free coordinate by its rate against the gradient's sign (less epsilon's share,
            # epsilon / sqrt(v) = 1e-7 / (0.0316 |g|), a few per cent at |g| = 1e-4)
            if t == 1:
                assert np.allclose(got[0, :3, 3] - c2w[0, :3, 3], -2e-3 * np.sign(g[0, :3]), atol=2e-4)
        rot, tr = pose_errors(po.poses, c2w)
        assert rot[1] < 1e-4 and tr[4] == 0 and rot[0] > 0.1 and tr[0] > 1e-3      # float32 storage: orthonormal to 1e-7
        back = PoseOptimizer(c2w, device="cpu", **hyper)
        back.load_state_dict(po.state_dict())
        assert torch.equal(back.poses, po.poses) and torch.equal(back._v, po._v) and back.step == 3 and back.fixed_views.tolist() == po.fixed_views.tolist()
    assert fixed_mask(None, 3).tolist() == [False] * 3
    for bad in ([3], [-1], [0.5], np.array([True, False]), [0, 1, 2]):
        with pytest.raises(ValueError):
            fixed_mask(bad, 3)
    with pytest.raises(ValueError):
        back.load_state_dict({"poses": c2w})
    with pytest.raises(ValueError):
        back.load_state_dict({**po.state_dict(), "poses": c2w[:2]})


class _Batches:
    def __init__(self, model=None):
        self.model, self.last_view, self.provider = model, None, None

    def set_cameras(self, provider):
        self.provider = provider

    def ray_model(self):
        return self.model

    def __iter__(self):
        raise AssertionError("nothing may be drawn before the arguments are checked")


def test_arguments_are_checked_on_the_host():
    from keras_nerf_amd import _lib, baked_pose
    from keras_nerf_amd.baked_pose import PoseOptimizer, check_pose_args, check_ray_model, fit_with_poses
    eye = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    good = dict(learning_rate_rotation=1e-3, learning_rate_translation=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
    assert check_pose_args((3, 4, 4), **good) == (1e-3, 1e-3, 0.9, 0.999, 1e-7)
    assert check_pose_args((3, 4, 4), **{**good, "learning_rate_rotation": 0.0})[0] == 0.0          # translation alone is a choice
    for shape in ((4, 4), (3, 3, 4), (0, 4, 4), (3, 4, 4, 1)):
        with pytest.raises(ValueError, match="c2w"):
            check_pose_args(shape, **good)
    for kw in (dict(learning_rate_rotation=-1.0), dict(learning_rate_rotation=0.0, learning_rate_translation=0.0), dict(beta_1=1.0),
               dict(beta_2=-0.1), dict(epsilon=0.0), dict(learning_rate_translation=float("nan")), dict(beta_1=True), dict(epsilon="1")):
        with pytest.raises(ValueError):
            check_pose_args((3, 4, 4), **{**good, **kw})
        with pytest.raises(ValueError):
            PoseOptimizer(eye, device="cpu", **{**good, **kw})
    with pytest.raises(ValueError, match="every view is fixed"):
        PoseOptimizer(eye, fixed_views=[0, 1, 2], device="cpu", **good)
    # NDC rays are refused; None and a pinhole model pass
    check_ray_model(None)
    check_ray_model(_lib.KnerfRayModel(0, _lib.SPACING_DISPARITY, 1.0))
    with pytest.raises(ValueError, match="NDC"):
        check_ray_model(_lib.KnerfRayModel(1, _lib.SPACING_LINEAR, 1.0))
    po = PoseOptimizer(eye, device="cpu", **good)
    field = object()
    with pytest.raises(ValueError, match="NDC"):
        po.accumulate(field, None, None, 0.0, 1.0, None, None, ray_model=_lib.KnerfRayModel(1, 0, 1.0))
    with pytest.raises(ValueError, match="NDC"):
        fit_with_poses(None, po, _Batches(_lib.KnerfRayModel(1, 0, 1.0)), 0.0, 1.0, field=field)
    with pytest.raises(ValueError, match="BakedField"):
        baked_pose.ray_gradients(field, None, None, 0.0, 1.0, None)
    for kw in (dict(steps=-1), dict(steps=1.5), dict(field_steps_first=-1), dict(field_steps_first=None), dict(field_steps_first=2)):
        with pytest.raises(ValueError):
            fit_with_poses(None, po, _Batches(), 0.0, 1.0, field=field, **kw)
    with pytest.raises(ValueError):
        fit_with_poses(None, po, _Batches(), 0.0, 1.0)                                           # neither optimiser nor field
    with pytest.raises(ValueError):
        fit_with_poses(None, object(), _Batches(), 0.0, 1.0, field=field)
    with pytest.raises(ValueError, match="set_cameras"):
        fit_with_poses(None, po, [], 0.0, 1.0, field=field)
    assert po.step == 0 and float(po.gradients().abs().max()) == 0.0


class _Loader:
    output_size = (4, 5)


class _Images:
    image_loader, image_paths = _Loader(), ["a", "b", "c"]


@pytest.mark.parametrize("steps_per_epoch", [None, 4])
def test_the_dataset_hook_leaves_the_schedule_alone(steps_per_epoch):
    from keras_nerf_amd.data.raybatch import RayBatchDataset
    plain, hooked = (RayBatchDataset(_Images(), 7, seed=3, steps_per_epoch=steps_per_epoch) for _ in range(2))
    assert plain._cameras is None and plain.last_view is None                                    # unset by default
    hooked.set_cameras(lambda: None)
    for _ in range(3):
        assert plain.schedule() == hooked.schedule()
    assert len(plain) == len(hooked) and (plain._perm, plain._step, plain._drawn) == (hooked._perm, hooked._step, hooked._drawn)
    hooked.set_cameras(None)
    assert hooked._cameras is None
    for bad in (3, "poses", np.eye(4)):
        with pytest.raises(ValueError):
            hooked.set_cameras(bad)
