"""Refining camera poses against a baked field on the GPU (keras_nerf_amd/baked_pose.py, csrc/baked_pose.hip) against
tests/baked_pose_reference.py: the per-ray gradients for every SH degree and lane variant, dense and through bricks of 4 and 8, on a
thin and an opaque lattice; bricks against dense bit for bit; the reduction to cameras; one optimiser step; a short refinement of
perturbed poses against a frozen field; the joint run's plumbing; refusals.  tests/README_baked_pose.md has what each test shows, the
bounds and the measured numbers.

The lattice and the 150 rays are those of tests/test_gpu_baked_train.py in kind (restated here): rays that cross the box, miss it, start
inside, have zero components, run parallel to an axis, have directions that are no unit vectors.

Preconditions, asserted on the fp64 reference alone before anything is compared (SEEDS were chosen on the CPU until they hold):
every fetched sample's raw colour channel and every hit ray's output keep MARGIN = 1e-4 from 0 and 1, with termination no
transmittance lies within 0.1 % of the threshold -- as in test_gpu_baked_train.py, for ALL rays.  The spatial gradient of a trilinear
field jumps from cell to cell, so a sample whose lattice coordinate lies closer to a cell boundary than the fp32 rounding of that
coordinate may sit in the neighbour cell on the GPU and take ITS gradient.  Rays with such a sample are left out of the comparison:
    u = ((o + d t) - lo) scale in fp32, eps = 2^-24:  t = near + (i + 1/2) step, two roundings at |t| <= 6.5: 13 eps;  d t: 13 eps |d_c| <= 13
    eps carried (a longer d has a shorter t) + 6.5 eps of its own;  + o near the box, |p| <= 1.2: 1.2 eps;  - lo: 2.1 eps;  in all 23 eps,
    times scale <= 6 / 1.3 = 4.6 cells per unit: 105 eps, + the product's own 8 eps: 113 eps = 6.7e-6 cell.
MARGIN_CELLS = 2e-5, three times that (a first estimate was 1e-4; the smaller threshold leaves fewer rays out).  The cap is a
condition, asserted: at most 5 % of the rays of a case are left out and the non-unit, inside-start and axis-parallel groups each keep
a ray.

Bound per gradient tensor over the compared rays: max(1e-5 x max |g_fp64|, 4 x max over 8 random summation orders of
|fp32 reference - fp64 reference|).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import baked_pose_reference as P
from tests import baked_train_reference as T

pytestmark = pytest.mark.gpu

RES = (9, 8, 7)
LO, HI = (-1.0, -0.8, -0.6), (1.0, 0.8, 0.7)
STEP = 0.04
N_RAYS = 150
MARGIN = 1e-4
MARGIN_CELLS = 2e-5
MAX_LEFT_OUT = 0.05
THIN, OPAQUE = 0.1, 1.0
TERMINATION = 1e-2
VARIANTS = {0: (0, 1), 1: (0, 1, 2), 2: (0, 1, 4), 3: (0, 1, 4)}      # lanes_per_ray values per degree (0: the default)
BRICKS = (4, 8)
SEEDS = {0: 4, 1: 4, 2: 4, 3: 4}                                       # per degree: chosen on the CPU until the preconditions hold
COEF_SCALE = {0: 0.6, 1: 0.6, 2: 0.4, 3: 0.3}        # about 1-10 % of the colour channels beyond a clamp edge, few close to one
GROUPS = {"inside-start": slice(110, 130), "axis-parallel": slice(138, 142), "non-unit": slice(142, 150)}


def _lattice(degree, dense):
    rng = np.random.default_rng(300 + SEEDS[degree])
    sigma = rng.uniform(0.0, 30.0, RES).astype(np.float32) * np.float32(dense)
    sigma[0], sigma[-1], sigma[:, 0], sigma[:, -1], sigma[:, :, 0], sigma[:, :, -1] = 0, 0, 0, 0, 0, 0     # no jump at the box face
    sigma[3:6, 2:4, 2:4] = 0                                                                              # empty interior cells
    sigma[6:] = 0                                                                                         # and two empty layers of cells
    K = (degree + 1) ** 2
    co = (rng.standard_normal(RES + (K, 3)) * COEF_SCALE[degree]).astype(np.float16)
    co[..., 0, :] += np.float16(1.5)
    return sigma, co


def _rays(degree):
    """150 rays: 0..89 cross the box from outside, 90..109 miss it, 110..129 start inside, 130..137 have one direction component
    exactly 0, 138..141 run parallel to an axis, 142..149 have directions that are no unit vectors; and one target colour per ray"""
    rng = np.random.default_rng(17 + 1000 * SEEDS[degree])
    lo, hi = np.array(LO), np.array(HI)
    mid = 0.5 * (lo + hi)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    o = mid + 3.0 * unit(rng.standard_normal((N_RAYS, 3)))
    aim = rng.uniform(lo + 0.1, hi - 0.1, (N_RAYS, 3))
    aim[:, 0] = rng.uniform(-0.9, 0.2, N_RAYS)                             # at the part of the box that holds density
    d = unit(aim - o)
    near, far = rng.uniform(0.0, 0.5, N_RAYS), rng.uniform(5.0, 6.5, N_RAYS)
    d[90:110] = unit(o[90:110] - mid + 0.3 * rng.standard_normal((20, 3)))
    o[110:130] = rng.uniform(lo + 0.05, hi - 0.05, (20, 3)); d[110:130] = unit(rng.standard_normal((20, 3))); near[110:130] = 0.0
    for i in range(130, 138):                                              # one component exactly 0
        a = i % 3
        t = rng.uniform(lo + 0.2, hi - 0.2)
        o[i][a] = t[a]
        d[i] = t - o[i]; d[i][a] = 0.0; d[i] = unit(d[i])
    for i in range(138, 142):                                              # parallel to an axis
        a = i % 3
        o[i] = rng.uniform(lo + 0.2, hi - 0.2); d[i] = 0.0; d[i][a] = 1.0 if i % 2 else -1.0
        o[i][a] = mid[a] - 3.0 * d[i][a]
    for i, s in zip(range(142, 150), (2.5, 0.3, 7.0, 1.0 / 3.0, 1.7, 0.6, 4.0, 0.45)):
        d[i] *= s; near[i] /= s; far[i] /= s
    target = rng.uniform(0.0, 1.0, (N_RAYS, 3))
    return {"o": o.astype(np.float32), "d": d.astype(np.float32), "near": near.astype(np.float32), "far": far.astype(np.float32),
            "target": target.astype(np.float32)}


_cases = {}


def _case(degree, dense, white, termination=0.0):
    """lattice, rays, the fp64 reference with its preconditions checked, the rays compared and the bounds: computed once per case"""
    key = (degree, dense, white, termination)
    if key in _cases:
        return _cases[key]
    sigma, co = _lattice(degree, dense)
    rays = _rays(degree)
    support = T.support_cells(sigma)
    args = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP, rays["target"], support, white,
            termination)
    info = {}
    L, go, gd = P.ray_gradients(*args, info=info)
    opa = info["opacity"]
    assert info["fetched"].sum() > 1500 and (opa[:90] > 0.05).all() and (opa[90:110] == 0).all()    # the set does what it says
    assert info["clamp_margin"].min() >= MARGIN, (key, "a raw colour or an output on a clamp edge", info["clamp_margin"].min())
    if termination:
        assert info["term_margin"].min() >= 1e-3, (key, "a transmittance on the threshold")
    keep = info["cell_margin"] >= MARGIN_CELLS
    left_out = int((~keep).sum())
    assert left_out <= MAX_LEFT_OUT * N_RAYS, (key, left_out)
    for name, sl in GROUPS.items():
        assert keep[sl].any(), (key, name)
        assert np.abs(go[sl][keep[sl]]).max() > 0 and np.abs(gd[sl][keep[sl]]).max() > 0, (key, name, "the group has no gradient")
    assert (go[90:110] == 0).all() and (gd[90:110] == 0).all()             # a ray that misses has none
    dev_o = dev_d = 0.0
    rng = np.random.default_rng(99)
    for _ in range(8):                                                     # the fp32 reference's own error over 8 summation orders
        _, o32, d32 = P.ray_gradients(*args, dtype=np.float32, order=rng)
        dev_o = max(dev_o, float(np.abs(o32 - go)[keep].max()))
        dev_d = max(dev_d, float(np.abs(d32 - gd)[keep].max()))
    bound = (max(1e-5 * float(np.abs(go[keep]).max()), 4.0 * dev_o), max(1e-5 * float(np.abs(gd[keep]).max()), 4.0 * dev_d))
    _cases[key] = {"sigma": sigma, "co": co, "rays": rays, "L": L, "go": go, "gd": gd, "keep": keep, "left_out": left_out, "bound": bound,
                   "dev": (dev_o, dev_d)}
    return _cases[key]


_fields = {}


def _fields_of(case_key):
    """the case's lattice as a dense field and as bricks of 4 and 8, built once"""
    if case_key not in _fields:
        from keras_nerf_amd.baked import BakedField
        case = _case(*case_key)
        dense = BakedField.from_arrays(case["sigma"], case["co"], (LO, HI))
        _fields[case_key] = {"dense": dense, **{f"bricks {b}": dense.compact(b) for b in BRICKS}}
    return _fields[case_key]


def _batch(rays, sl=slice(None)):
    return rays["o"][sl], rays["d"][sl], rays["near"][sl], rays["far"][sl], rays["target"][sl]


CASES = [(deg, dense, white, 0.0) for deg in (0, 1, 2, 3) for dense in (THIN, OPAQUE) for white in (False, True)] + \
    [(deg, OPAQUE, deg % 2 == 1, TERMINATION) for deg in (0, 1, 2, 3)]


@pytest.mark.parametrize("degree,dense,white,termination", CASES)
def test_ray_gradients_match_fp64(degree, dense, white, termination):
    key = (degree, dense, white, termination)
    case = _case(*key)
    keep, rays = case["keep"], case["rays"]
    fields = _fields_of(key)
    opt = fields["dense"].optimizer(0.05, 0.01, step=STEP, white_background=white, termination=termination)
    train_loss = float(opt.accumulate(*_batch(rays)))
    for lanes in VARIANTS[degree]:
        for name, field in fields.items():
            go, gd, loss = field.ray_gradients(*_batch(rays), step=STEP, white_background=white, termination=termination, lanes_per_ray=lanes)
            assert loss.dtype == torch.float64 and loss.dim() == 0 and go.dtype == torch.float32 and tuple(go.shape) == (N_RAYS, 3)
            go, gd = go.cpu().numpy(), gd.cpu().numpy()
            err = (float(np.abs(go - case["go"])[keep].max()), float(np.abs(gd - case["gd"])[keep].max()))
            print(f"degree {degree} dense {dense} white {white} termination {termination} lanes {lanes} {name}: max |g - fp64| origin "
                  f"{err[0]:.3e} (bound {case['bound'][0]:.3e}, fp32 reference {case['dev'][0]:.3e}, max |g| "
                  f"{np.abs(case['go'][keep]).max():.3e}), direction {err[1]:.3e} (bound {case['bound'][1]:.3e}, fp32 reference "
                  f"{case['dev'][1]:.3e}, max |g| {np.abs(case['gd'][keep]).max():.3e}); {case['left_out']} of {N_RAYS} rays left out; "
                  f"loss {float(loss):.6e} (fp64 {case['L']:.6e}, accumulate {train_loss:.6e})")
            assert np.isfinite(go).all() and np.isfinite(gd).all()
            assert (go[90:110] == 0).all() and (gd[90:110] == 0).all()     # zeros are written where nothing contributes
            assert abs(float(loss) - train_loss) <= 1e-5 * train_loss, (lanes, name, float(loss), train_loss)
            assert abs(float(loss) - case["L"]) <= 1e-5 * case["L"]
            assert err[0] <= case["bound"][0], (lanes, name, "origin", err[0], case["bound"][0])
            assert err[1] <= case["bound"][1], (lanes, name, "direction", err[1], case["bound"][1])


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_bricks_equal_dense_bit_for_bit(degree):
    for key in ((degree, THIN, True, 0.0), (degree, OPAQUE, degree % 2 == 1, TERMINATION)):
        rays = _case(*key)["rays"]
        fields = _fields_of(key)
        for b in BRICKS:
            bricks = fields[f"bricks {b}"]
            dense = bricks.to_dense()
            assert bricks.n_bricks < int(np.prod(bricks.brick_of.shape)) or b == 8      # some brick is absent (b = 4)
            for lanes in VARIANTS[degree]:
                kw = dict(step=STEP, white_background=key[2], termination=key[3], lanes_per_ray=lanes)
                a, c = bricks.ray_gradients(*_batch(rays), **kw), dense.ray_gradients(*_batch(rays), **kw)
                for x, y, what in zip(a, c, ("grad_origin", "grad_direction", "loss")):
                    assert torch.equal(x, y), (key, b, lanes, what)
                again = bricks.ray_gradients(*_batch(rays), **kw)
                assert torch.equal(a[0], again[0]) and torch.equal(a[1], again[1])       # no atomics: the same bits every time


def test_pose_reduction():
    """against the fp64 reference on random per-ray gradients: uneven view counts, an empty view, indices out of range"""
    from keras_nerf_amd import baked_pose
    rng = np.random.default_rng(5)
    n, V = 1777, 7
    go, gd, d = (rng.standard_normal((n, 3)).astype(np.float32) * s for s in (1e-3, 2e-3, 1.7))
    view = rng.choice([0, 1, 2, 4, 5, 6], size=n, p=[0.4, 0.05, 0.25, 0.1, 0.15, 0.05]).astype(np.int32)      # view 3 has no ray
    view[::97] = -1
    view[5::131] = V
    view[7::211] = 2 ** 31 - 1
    ref = P.pose_gradients(go, gd, d, view, V)
    dev = torch.device("cuda")
    t = lambda x: torch.as_tensor(x).to(dev)
    out = baked_pose.pose_gradients(t(go), t(gd), t(d), t(view), V)
    assert out.dtype == torch.float64 and tuple(out.shape) == (V, 6)
    got = out.cpu().numpy()
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"pose reduction: max |out - fp64| {err:.3e}, largest entry {top:.3e}, bound {1e-12 * top:.3e}")
    assert (got[3] == 0).all() and np.abs(got[[0, 1, 2, 4, 5, 6]]).min() > 0
    assert err <= 1e-12 * top
    assert torch.equal(out, baked_pose.pose_gradients(t(go), t(gd), t(d), t(view), V))
    assert torch.equal(out, baked_pose.pose_gradients(t(go), t(gd), t(d), t(view.astype(np.int64)), V))       # any integer type
    one = baked_pose.pose_gradients(t(go), t(gd), t(d), t(view), 1).cpu().numpy()                             # fewer views: the rest is skipped
    assert np.array_equal(one[0], got[0])


def _random_poses(rng, V):
    c2w = np.tile(np.eye(4), (V, 1, 1))
    c2w[:, :3, :3] = P.rodrigues(rng.standard_normal((V, 3)))
    c2w[:, :3, 3] = rng.uniform(-3, 3, (V, 3))
    return c2w.astype(np.float32)


@pytest.mark.parametrize("before", [0, 2])
def test_one_optimiser_step(before):
    """poses and moments after accumulate + apply against pose_adam_step fed the kernel's own [V,6] gradient; before = 2: step 3"""
    from keras_nerf_amd.baked_pose import PoseOptimizer
    key = (2, THIN, True, 0.0)
    rays, field = _case(*key)["rays"], _fields_of(key)["dense"]
    rng = np.random.default_rng(11)
    V = 5
    c2w = _random_poses(rng, V)
    view = rng.integers(0, V, N_RAYS).astype(np.int32)
    hyper = dict(learning_rate_rotation=3e-3, learning_rate_translation=2e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
    po = PoseOptimizer(c2w, fixed_views=[3], **hyper)
    assert po.poses.dtype == torch.float32 and np.array_equal(po.poses.cpu().numpy().view(np.uint32), c2w.view(np.uint32))
    live = po.poses
    kw = dict(step=STEP, white_background=True)
    for _ in range(before):
        po.accumulate(field, *_batch(rays), view, **kw)
        po.apply()
    loss = po.accumulate(field, *_batch(rays), view, **kw)
    g = po.gradients().cpu().numpy()
    assert g.dtype == np.float64 and g.shape == (V, 6) and np.abs(g).min() > 0
    go, gd, loss2 = field.ray_gradients(*_batch(rays), **kw)
    assert torch.equal(loss, loss2)
    assert np.array_equal(g, P.pose_gradients(go.cpu().numpy(), gd.cpu().numpy(), rays["d"], view, V)) or \
        np.abs(g - P.pose_gradients(go.cpu().numpy(), gd.cpu().numpy(), rays["d"], view, V)).max() <= 1e-12 * np.abs(g).max()
    start, m0, v0 = po.poses.cpu().numpy().astype(np.float64), po._m.cpu().numpy(), po._v.cpu().numpy()
    fixed = np.arange(V) == 3
    want, m1, v1 = P.pose_adam_step(start, m0, v0, g, hyper["learning_rate_rotation"], hyper["learning_rate_translation"], 0.9, 0.999, 1e-7,
                                    before + 1, fixed=fixed)
    po.apply()
    assert po.step == before + 1 and po.poses is live and float(po.gradients().abs().max()) == 0.0
    got = po.poses.cpu().numpy()
    # the stored matrix is the float64 result rounded to float32 once: half an ulp of the entry, and the float64 arithmetic's own 1e-15
    tol = 2.0 ** -24 * np.maximum(np.abs(want), 2.0 ** -126) + 1e-14
    err = np.abs(got.astype(np.float64) - want)
    moved = np.abs(got.astype(np.float64) - start)[~fixed][:, :3, :].max()
    print(f"step {before + 1}: max |pose - fp64| {err.max():.3e} (largest allowance {tol.max():.3e}), the step moved an entry by up to {moved:.3e}")
    assert (err <= tol).all(), (err.max(), tol.max())
    assert moved > 1e-4
    assert np.array_equal(got[3].view(np.uint32), c2w[3].view(np.uint32))                       # the fixed view, bit for bit
    assert (po._m.cpu().numpy()[3] == 0).all() and (po._v.cpu().numpy()[3] == 0).all()
    assert np.abs(po._m.cpu().numpy() - m1).max() <= 1e-13 * np.abs(m1).max() and np.abs(po._v.cpu().numpy() - v1).max() <= 1e-13 * np.abs(v1).max()
    rot = got[:, :3, :3].astype(np.float64)
    assert np.abs(rot @ np.transpose(rot, (0, 2, 1)) - np.eye(3)).max() < 1e-6                  # float32 storage of an orthonormal matrix
    state = po.state_dict()
    other = PoseOptimizer(c2w, **hyper)
    other.load_state_dict(state)
    assert torch.equal(other.poses, po.poses) and torch.equal(other._m, po._m) and other.step == po.step and bool(other.fixed_views[3])


# ---- a smooth scene with cameras around it
SCENE_RES, SCENE_BOUNDS, SCENE_STEP = 24, ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), 0.04
SCENE_VIEWS, SCENE_PIXELS, SCENE_FOCAL, SCENE_NEAR, SCENE_FAR = 5, 24, 30.0, 1.5, 4.5


def _scene():
    """a few Gaussian blobs of density with smoothly varying degree-1 colour on a 24^3 lattice"""
    from keras_nerf_amd.baked import BakedField
    ax = np.linspace(-1.0, 1.0, SCENE_RES)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    sigma = np.zeros_like(x)
    for (cx, cy, cz), s, a in (((0.3, 0.1, -0.2), 0.22, 9.0), ((-0.35, -0.2, 0.25), 0.18, 12.0), ((0.0, 0.4, 0.3), 0.2, 8.0),
                               ((-0.1, -0.45, -0.35), 0.16, 10.0)):
        sigma += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * s * s))
    sigma[sigma < 0.05] = 0.0
    sigma[0], sigma[-1], sigma[:, 0], sigma[:, -1], sigma[:, :, 0], sigma[:, :, -1] = 0, 0, 0, 0, 0, 0
    co = np.zeros((SCENE_RES,) * 3 + (4, 3), dtype=np.float32)
    y0 = 0.28209479177387814
    co[..., 0, 0] = (0.5 + 0.35 * np.sin(3.0 * x + 1.0)) / y0
    co[..., 0, 1] = (0.5 + 0.35 * np.sin(2.5 * y - 0.5)) / y0
    co[..., 0, 2] = (0.5 + 0.35 * np.cos(3.5 * z)) / y0
    co[..., 1, :] = 0.2 * np.stack([x, y, z], axis=-1)
    co[..., 3, :] = 0.2 * np.stack([z, x, y], axis=-1)
    return BakedField.from_arrays(sigma.astype(np.float32), co.astype(np.float16), SCENE_BOUNDS)


def _look_at(eye):
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0])); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, -fwd, eye
    return c2w


def _true_poses():
    ang = np.linspace(0.0, 2.0 * np.pi, SCENE_VIEWS, endpoint=False) + 0.3
    return np.stack([_look_at(3.0 * np.array([np.cos(a) * 0.9, np.sin(a) * 0.9, 0.45 * (-1) ** i])) for i, a in enumerate(ang)]).astype(np.float32)


def _perturbed(c2w, seed, degrees=1.5, shift=0.04):
    """every pose turned by `degrees` about a random axis and moved by `shift` (0.02 of the scene's size of 2) in a random direction"""
    rng = np.random.default_rng(seed)
    V = c2w.shape[0]
    axis = rng.standard_normal((V, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    move = rng.standard_normal((V, 3)); move /= np.linalg.norm(move, axis=1, keepdims=True)
    return P.move_poses(c2w, np.radians(degrees) * axis, shift * move).astype(np.float32)


def _camera_rays(c2w):
    """pinhole rays of every pixel of every view, o = t, d = R cam (not normalised), on the device: (o [n,3], d [n,3], view int32 [n])"""
    dev = c2w.device
    px = torch.arange(SCENE_PIXELS, device=dev, dtype=torch.float32) + 0.5 - SCENE_PIXELS / 2
    v, u = torch.meshgrid(px, px, indexing="ij")
    cam = torch.stack([u / SCENE_FOCAL, -v / SCENE_FOCAL, -torch.ones_like(u)], dim=-1).reshape(-1, 3)
    d = torch.einsum("vab,pb->vpa", c2w[:, :3, :3], cam)
    o = c2w[:, None, :3, 3].expand_as(d)
    view = torch.arange(c2w.shape[0], device=dev, dtype=torch.int32)[:, None].expand(d.shape[:2])
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), view.reshape(-1).contiguous()


class _Batches:
    """what fit_with_poses needs of a RayBatchDataset: every batch holds all pixels of all views, drawn with the provider's poses"""

    def __init__(self, target, n_batches, model=None):
        self.target, self.n_batches, self.model = target, n_batches, model
        self.provider, self.last_view = None, None

    def set_cameras(self, provider):
        self.provider = provider

    def ray_model(self):
        return self.model

    def __iter__(self):
        for _ in range(self.n_batches):
            o, d, self.last_view = _camera_rays(self.provider())
            yield self.target, (o, d, None)


_scene_cache = {}


def _scene_and_target():
    if not _scene_cache:
        field = _scene()
        truth = _true_poses()
        o, d, _ = _camera_rays(torch.as_tensor(truth).to(field.device))
        out = field.render(o, d, SCENE_NEAR, SCENE_FAR, step=SCENE_STEP, outputs=("image", "opacity"))
        assert 0.2 < float((out["opacity"] > 0.5).float().mean()) < 0.95                       # the views see the blobs, and around them
        _scene_cache.update(field=field, truth=truth, target=out["image"])
    return _scene_cache["field"], _scene_cache["truth"], _scene_cache["target"]


REFINE_STEPS = 60
# measured on an MI355X over the seeds 0, 1, 2 (tests/README_baked_pose.md has the three runs): final / initial after REFINE_STEPS steps;
# the assertion asks for half of the SMALLEST measured improvement in log terms, i.e. ratio <= sqrt(largest measured ratio)
REFINE_MEASURED = {"loss": 0.0071, "rotation": 0.5381, "translation": 0.7687}       # the largest (worst) of the three seeds each


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_it_refines(seed):
    """poses only, the field frozen: cameras perturbed by 1.5 degrees and 0.02 of the scene's size find their way back"""
    from keras_nerf_amd.baked_pose import PoseOptimizer, pose_errors
    field, truth, target = _scene_and_target()
    start = _perturbed(truth, seed)
    po = PoseOptimizer(start, learning_rate_rotation=2e-3, learning_rate_translation=3e-3)
    r0, t0 = (e.mean() for e in pose_errors(start, truth))
    losses = []
    for _ in range(REFINE_STEPS):
        o, d, view = _camera_rays(po.poses)
        losses.append(po.accumulate(field, o, d, SCENE_NEAR, SCENE_FAR, target, view, step=SCENE_STEP))
        po.apply()
    o, d, view = _camera_rays(po.poses)
    final = float(field.ray_gradients(o, d, SCENE_NEAR, SCENE_FAR, target, step=SCENE_STEP)[2])
    first = float(losses[0])
    r1, t1 = (e.mean() for e in pose_errors(po.poses, truth))
    ratios = {"loss": final / first, "rotation": r1 / r0, "translation": t1 / t0}
    print(f"seed {seed}: loss {first:.4e} -> {final:.4e} (x {ratios['loss']:.4f}), mean rotation error {r0:.3f} -> {r1:.3f} degrees "
          f"(x {ratios['rotation']:.4f}), mean translation error {t0:.4f} -> {t1:.4f} (x {ratios['translation']:.4f})")
    assert 1.0 < r0 < 2.0 and 0.03 < t0 < 0.05 and all(np.isfinite(float(x)) for x in losses)
    for what, ratio in ratios.items():
        assert ratio < 1.0, (what, ratio)
        assert ratio <= np.sqrt(REFINE_MEASURED[what]), (what, ratio, REFINE_MEASURED[what])


@pytest.mark.parametrize("kind", ["dense", "bricks"])
def test_joint_run_plumbing(kind):
    from keras_nerf_amd import baked_pose, baked_train
    from keras_nerf_amd.baked import BakedField, BrickBakedField
    field, truth, target = _scene_and_target()
    start = _perturbed(truth, 7)
    if kind == "dense":
        opt = field.optimizer(0.05, 0.01, step=SCENE_STEP, dilation=1)
    else:
        opt = baked_train.brick_optimizer(field.compact(8), 0.05, 0.01, step=SCENE_STEP, dilation=1)
    records0 = opt.field._records.clone()
    po = baked_pose.PoseOptimizer(start, 2e-3, 3e-3, fixed_views=[0])
    batches = _Batches(target, 6)
    hist = baked_pose.fit_with_poses(opt, po, batches, SCENE_NEAR, SCENE_FAR, steps=5, field_steps_first=2)
    assert len(hist["loss"]) == 5 and np.isfinite(hist["loss"]).all() and opt.iterations == 5 and po.step == 3
    assert not torch.equal(opt.field._records, records0)                                    # the field's records moved
    got = po.poses.cpu().numpy()
    assert np.array_equal(got[0].view(np.uint32), start[0].view(np.uint32))                 # the fixed view did not
    assert all(np.abs(got[v] - start[v]).max() > 1e-4 for v in range(1, SCENE_VIEWS))      # every other pose did
    assert batches.last_view is not None and batches.last_view.dtype == torch.int32
    done = opt.finish()
    assert type(done) is (BakedField if kind == "dense" else BrickBakedField)
    o, d, _ = _camera_rays(po.poses)
    img = done.render(o, d, SCENE_NEAR, SCENE_FAR, step=SCENE_STEP, outputs="image")["image"]
    assert bool(torch.isfinite(img).all()) and float(img.max()) > 0.1
    # poses only, against a frozen field, through the same entry point
    alone = baked_pose.PoseOptimizer(start, 2e-3, 3e-3)
    hist = baked_pose.fit_with_poses(None, alone, _Batches(target, 3), SCENE_NEAR, SCENE_FAR, field=done, step=SCENE_STEP)
    assert len(hist["loss"]) == 3 and np.isfinite(hist["loss"]).all() and alone.step == 3


def test_arguments_are_refused_before_any_launch():
    from keras_nerf_amd import _lib, baked_pose
    from keras_nerf_amd.baked import _stream
    from keras_nerf_amd.runtime import _ptr
    key = (1, THIN, False, 0.0)
    rays, fields = _case(*key)["rays"], _fields_of(key)
    o, d, near, far, tg = _batch(rays)
    view = np.zeros(N_RAYS, dtype=np.int32)
    for field in fields.values():
        for bad in (tg[:100], tg[:, :2], tg.reshape(-1)):
            with pytest.raises(ValueError, match="target"):
                field.ray_gradients(o, d, near, far, bad, step=STEP)
        for kw in (dict(step=0.0), dict(termination=1.0), dict(lanes_per_ray=4), dict(n_total=0)):
            with pytest.raises(ValueError):
                field.ray_gradients(o, d, near, far, tg, **{**dict(step=STEP), **kw})
        with pytest.raises(ValueError):
            field.ray_gradients(o, d[:10], near, far, tg, step=STEP)
    dense = fields["dense"]
    dev = dense.device
    # the entry points themselves: NULL outputs, an unknown flag bit, a lane count the degree does not have, a bad step
    t = lambda x: torch.as_tensor(x).to(dev)
    to, td, tt = t(o), t(d), t(tg)
    go, gd = torch.full((N_RAYS, 3), 7.0, device=dev), torch.full((N_RAYS, 3), 7.0, device=dev)
    lib = _lib.load()
    for entry, fld in ((lib.knerf_baked_ray_gradients, dense), (lib.knerf_baked_ray_gradients_bricks, fields["bricks 4"])):
        call = lambda step=STEP, flags=2, out_o=go, out_d=gd, target=tt: entry(
            _stream(dev), C.byref(fld._c), _ptr(to), _ptr(td), None, None, 0.0, 6.0, _ptr(target), N_RAYS, 0, step, 0.0, flags, _ptr(out_o),
            _ptr(out_d), None)
        assert call(out_o=None) == _lib.KNERF_ERR_INVALID and call(out_d=None) == _lib.KNERF_ERR_INVALID
        assert call(target=None) == _lib.KNERF_ERR_INVALID and call(step=0.0) == _lib.KNERF_ERR_INVALID
        assert call(flags=2 | 64) == _lib.KNERF_ERR_INVALID and call(flags=2 | (4 << 8)) == _lib.KNERF_ERR_INVALID
    assert lib.knerf_pose_gradients(_stream(dev), _ptr(go), _ptr(gd), _ptr(td), None, N_RAYS, 3, None) == _lib.KNERF_ERR_INVALID
    assert float(go.min()) == 7.0 and float(gd.max()) == 7.0                                  # nothing was launched
    with pytest.raises(ValueError, match="integers"):
        baked_pose.pose_gradients(go, gd, td, torch.zeros(N_RAYS, device=dev), 3)
    with pytest.raises(ValueError):
        baked_pose.pose_gradients(go, gd, td, t(view[:10]), 3)
    po = baked_pose.PoseOptimizer(np.tile(np.eye(4, dtype=np.float32), (3, 1, 1)), 1e-3, 1e-3)
    ndc = _lib.KnerfRayModel(1, _lib.SPACING_LINEAR, 1.0)
    with pytest.raises(ValueError, match="NDC"):
        po.accumulate(dense, o, d, near, far, tg, view, step=STEP, ray_model=ndc)
    with pytest.raises(ValueError, match="NDC"):
        baked_pose.fit_with_poses(None, po, _Batches(tt, 2, model=ndc), 0.0, 6.0, field=dense, step=STEP)
    assert float(po.gradients().abs().max()) == 0.0 and po.step == 0
    po.accumulate(dense, o, d, near, far, tg, view, step=STEP, ray_model=_lib.KnerfRayModel(0, _lib.SPACING_LINEAR, 1.0))   # pinhole passes
    with pytest.raises(ValueError):
        baked_pose.fit_with_poses(None, po, [(tt, (to, td, None))], 0.0, 6.0, field=dense)     # batches that cannot follow the poses
    with pytest.raises(ValueError):
        baked_pose.fit_with_poses(None, po, _Batches(tt, 2), 0.0, 6.0)                         # neither an optimiser nor a field


def test_the_dataset_hook_is_additive(tmp_path):
    """RayBatchDataset.set_cameras: unset, the batches are what they were; with the dataset's own matrices as provider the rays are
    the same bits and last_view names each ray's camera; with other matrices the rays follow them"""
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.runtime import draw_ray_batch
    from tests.synthetic_scene import write
    root = write(str(tmp_path / "scene"), n=(6, 2, 3))
    load = lambda: DatasetLoader(root, white_background=True).load_dataset(1, 24, 24, 2.0, 6.0, 64)[0]
    plain, hooked, moved = (load().ray_batches(1024, seed=4) for _ in range(3))
    assert plain.last_view is None and plain.ray_model() is None
    with pytest.raises(ValueError):
        hooked.set_cameras(3)
    cams = hooked._resident_all()[1]
    asked = []
    hooked.set_cameras(lambda: (asked.append(1), cams)[1])
    shifted = cams.clone()
    shifted[:, :3, 3] += 0.25
    moved.set_cameras(lambda: shifted)
    n = 0
    for (ta, (oa, da, tsa)), (tb, (ob, db, tsb)), (tc, (oc, dc, _)) in zip(plain, hooked, moved):
        assert torch.equal(ta, tb) and torch.equal(oa, ob) and torch.equal(da, db) and torch.equal(tsa, tsb)
        assert torch.equal(tc, ta) and torch.equal(dc, da) and torch.equal(oc, oa + 0.25)
        perm, first, count = hooked.last_draw
        index = draw_ray_batch(*hooked._resident_all(), hooked._rg.focal_length, 2.0, 6.0, 64, 4, perm, first, count, want_index=True)[4]
        assert hooked.last_view.dtype == torch.int32 and torch.equal(hooked.last_view.to(torch.int64), index // (24 * 24))
        assert torch.equal(ob, cams[hooked.last_view.long(), :3, 3])                            # o = t of the ray's own camera
        n += 1
    assert n == 3 == len(asked) and plain.last_view is None
    assert plain.schedule() == hooked.schedule()                                               # and the schedule went the same way
    hooked.set_cameras(None)
    assert hooked.last_view is None
