"""Depth supervision of the baked-field optimisers without a GPU: the fp64 reference's own gradient against central differences (the
reference is checked independently of any kernel), the keyword refusals, which entry point an accumulate() reaches with and without
depth (the library stubbed as in tests/test_baked_optimizer_calls_host.py), RayBatchDataset.set_depth's shape checks, and the unit
conversions of keras_nerf_amd/data/depth.py against closed forms."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from keras_nerf_amd import _lib, baked_bricks_grow, baked_bricks_train, baked_train, losses
from keras_nerf_amd.baked import BakedField, BrickBakedField
from keras_nerf_amd.baked_train import TERM_NAMES, check_objective
from tests import baked_depth_reference as D
from tests import baked_objective_reference as Q
from tests import baked_rgba_reference as P
from tests import baked_train_reference as T
from tests import test_baked_optimizer_calls_host as H

# ---- the reference against central differences
RES, LO, HI, STEP = (5, 4, 4), (-1.0, -0.8, -0.8), (1.0, 0.8, 0.8), 0.11


def _scene(degree=1, n=24, seed=0):
    rng = np.random.default_rng(seed)
    sigma = rng.uniform(0.5, 6.0, RES)
    sigma[0], sigma[-1], sigma[:, 0], sigma[:, -1], sigma[:, :, 0], sigma[:, :, -1] = 0, 0, 0, 0, 0, 0
    K = (degree + 1) ** 2
    co = rng.standard_normal(RES + (K, 3)) * 0.15
    co[..., 0, :] += 1.4                                                   # colours well inside (0, 1): no clamp edge nearby
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    o = 3.0 * unit(rng.standard_normal((n, 3)))
    d = unit(rng.uniform(-0.4, 0.4, (n, 3)) - o) * rng.uniform(0.5, 2.0, (n, 1))
    o, d = o.astype(np.float32), d.astype(np.float32)
    near = np.zeros(n, np.float32)
    far = (6.0 / np.linalg.norm(d, axis=1)).astype(np.float32)
    target = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    bg = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    alpha = rng.uniform(0.1, 0.9, n).astype(np.float32)
    return sigma, co, o, d, near, far, target, bg, alpha


@pytest.mark.parametrize("name,objective", [("mse", dict(loss_kind=Q.MSE)),
                                            ("full", dict(loss_kind=Q.HUBER, huber_delta=0.2, distortion=0.3, opacity_entropy=0.05, opacity=0.2))])
def test_reference_gradient_matches_central_differences(name, objective):
    sigma, co, o, d, near, far, target, bg, alpha = _scene()
    support = T.support_cells(sigma.astype(np.float32))
    n = o.shape[0]
    probe = {}
    D.loss_and_grad(sigma, co, LO, HI, o, d, near, far, STEP, target, support, info=probe)
    Z = probe["Z"]
    assert (Z > 0).sum() >= n // 2
    rng = np.random.default_rng(1)
    z = np.where(Z > 0, Z * (1.0 + np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * rng.uniform(0.05, 0.3, n)), 2.0).astype(np.float32)
    c = rng.uniform(0.1, 2.0, n).astype(np.float32)
    c[::3] = 0.0
    z[c == 0] = np.nan
    kw = dict(background=bg if name == "full" else None, alpha=alpha if name == "full" else None, depth_target=z, depth_weight=c, depth=0.7,
              **objective)
    f = lambda s, k: D.loss_and_grad(s, k, LO, HI, o, d, near, far, STEP, target, support, **kw)
    L, terms, gs, gc = f(sigma, co)
    base = P.loss_and_grad(sigma, co, LO, HI, o, d, near, far, STEP, target, support, background=kw["background"], alpha=kw["alpha"], **objective)
    assert terms["depth"] > 0 and np.isfinite(L) and np.isclose(L, base[0] + float(np.float32(0.7)) * terms["depth"], rtol=1e-14)
    assert np.abs(gs - base[2]).max() > 1e-3 * np.abs(gs).max()            # the depth term's share is there
    assert np.array_equal(gc, base[3])                                     # ... and the colours have none of it
    # mirror: the kernel's summation order is the same function
    Lm, _, gsm, gcm = D.loss_and_grad(sigma, co, LO, HI, o, d, near, far, STEP, target, support, mirror=True, **kw)
    assert abs(Lm - L) <= 1e-14 * abs(L) and np.abs(gsm - gs).max() <= 1e-12 * np.abs(gs).max() and np.array_equal(gcm, gc)
    trainable = np.argwhere(np.abs(gs) > 0.05 * np.abs(gs).max())
    picks = [tuple(trainable[i]) for i in rng.choice(len(trainable), 5, replace=False)]
    for p in picks:
        h = 1e-5
        sp, sm = sigma.copy(), sigma.copy()
        sp[p] += h; sm[p] -= h
        num = (f(sp, co)[0] - f(sm, co)[0]) / (2 * h)
        assert abs(num - gs[p]) <= 1e-6 * abs(gs[p]), (name, "sigma", p, num, gs[p])
    weighed = np.argwhere(np.abs(gc) > 0.05 * np.abs(gc).max())
    for i in rng.choice(len(weighed), 5, replace=False):
        p = tuple(weighed[i])
        h = 1e-5
        cp, cm = co.copy(), co.copy()
        cp[p] += h; cm[p] -= h
        num = (f(sigma, cp)[0] - f(sigma, cm)[0]) / (2 * h)
        assert abs(num - gc[p]) <= 1e-6 * abs(gc[p]), (name, "coefficient", p, num, gc[p])


def test_reference_weight_zero_is_no_depth_and_optimise_descends():
    sigma, co, o, d, near, far, target, bg, alpha = _scene(degree=0, n=12)
    support = T.support_cells(sigma.astype(np.float32))
    geo = (LO, HI, o, d, near, far, STEP, target, support)
    n = o.shape[0]
    a = P.loss_and_grad(sigma, co, *geo)
    b = D.loss_and_grad(sigma, co, *geo, depth_target=np.full(n, np.nan, np.float32), depth_weight=np.zeros(n, np.float32), depth=0.5)
    assert a[0] == b[0] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and b[1]["depth"] == 0.0
    assert tuple(b[1]) == D.TERMS == P.TERMS + ("depth",)
    values = D.optimise(sigma.astype(np.float32), co.astype(np.float16), *geo[:-1], 0.05, 0.01, 3, depth_target=np.full(n, 2.0, np.float32), depth=0.5)
    assert len(values) == 4 and values[-1] < values[0]


# ---- keywords
def _constructors():
    return [(BakedField.optimizer, BakedField), (baked_train.BakedFieldOptimizer, BakedField), (baked_train.brick_optimizer, BrickBakedField),
            (baked_bricks_train.BrickFieldOptimizer, BrickBakedField), (baked_bricks_grow.grid_trainer, BrickBakedField),
            (baked_bricks_grow.BrickGridTrainer, BrickBakedField)]


def test_depth_loss_is_checked_before_anything_else(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    for make, source_type in _constructors():
        source = object.__new__(source_type)                               # nothing behind it: touching it is an AttributeError
        for bad in (-1e-3, float("nan"), float("inf"), -float("inf"), "0.1", object(), True, 1e39, [0.1]):
            with pytest.raises(ValueError, match="depth_loss"):
                make(source, 0.05, 0.01, depth_loss=bad)


def test_depth_loss_arrives_under_its_own_name(monkeypatch):
    """through every constructor and factory, beside every other keyword (the sentinels of test_baked_optimizer_calls_host.py)"""
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    import inspect
    sent = H._sentinels(False)
    for make, source_type in _constructors():
        source = object.__new__(source_type)
        source.sh_degree = 2
        names = list(inspect.signature(make).parameters)[1:]
        with pytest.raises(AttributeError) as err:
            make(source, **{k: sent[k] for k in names}, depth_loss=0.23)
        opt = H._optimizer_in(err.value)
        # a factory sets the value on the optimiser it returns, so only the classes hold it while they are under construction
        if isinstance(make, type):
            assert opt.depth_loss == 0.23, make
        assert opt._rgba.opacity == 0.19
    assert baked_train.GridOptimizer.depth_loss == 0.0


# ---- the launch path, the library stubbed
lib = H.lib
DEPTH = len(_lib.SIGNATURES["knerf_baked_train_rays_rgba"][1])              # the position of the depth record
H.STRUCTS[C.POINTER(_lib.KnerfBakedDepth)] = ("target", "weight", "depth")


def _bare(cls, objective=None, depth_loss=0.0, **rgba):
    opt = H.bare(cls, objective, **rgba)
    if depth_loss is not None:
        opt.depth_loss = depth_loss
    return opt


@pytest.mark.parametrize("cls,stem,_tv,_apply", H.CLASSES)
@pytest.mark.parametrize("route,objective_kw,rgba_kw,columns,per_call", H.ROUTES)
def test_without_depth_the_call_is_the_one_made_today(lib, cls, stem, _tv, _apply, route, objective_kw, rgba_kw, columns, per_call):
    """depth_loss = 0 with depth tensors given, and an optimiser that never heard of the keyword (the class default), make the same call
    with the same converted arguments as accumulate() without depth"""
    o, d, far = H.rays()
    target = np.full((H.N, columns), 0.5, np.float32)
    extra = dict(background=np.full((H.N, 3), 0.25, np.float32)) if per_call else {}
    objective = check_objective(objective_kw.get("loss"), objective_kw.get("regularizers"))
    z, c = np.linspace(1.0, 2.0, H.N, dtype=np.float32), np.ones(H.N, np.float32)
    seen = []
    for depth_loss, depth_kw in ((None, {}), (0.0, {}), (0.0, dict(depth=z, depth_weight=c)), (None, dict(depth=z))):
        lib.calls.clear()
        opt = _bare(cls, objective, depth_loss, white_background=True, **rgba_kw)
        opt.accumulate(o, d, H.NEAR, far, target, n_total=H.N_TOTAL, **extra, **depth_kw)
        assert lib.names == [stem + route]
        a = lib.calls[0][1]
        pointers = {H.O, H.D, H.FAR_T, H.TARGET, H.SQ, H.TERMS}
        seen.append([bool(v) if i in pointers else ({k: (bool(x) if k in ("background", "alpha") else x) for k, x in v.items()} if isinstance(v, dict) else v)
                     for i, v in enumerate(a)])
        assert tuple(opt.objective_terms() or ()) == (() if not route else TERM_NAMES + (("opacity",) if route == "_rgba" else ()))
    assert all(s == seen[0] for s in seen[1:])


@pytest.mark.parametrize("cls,stem,_tv,_apply", H.CLASSES)
@pytest.mark.parametrize("route,objective_kw,rgba_kw,columns,per_call", H.ROUTES)
@pytest.mark.parametrize("weighted", [True, False])
def test_with_depth_the_call_is_the_depth_entry_point(lib, cls, stem, _tv, _apply, route, objective_kw, rgba_kw, columns, per_call, weighted):
    o, d, far = H.rays()
    target = np.full((H.N, columns), 0.5, np.float32)
    extra = dict(background=np.full((H.N, 3), 0.25, np.float32)) if per_call else {}
    objective = check_objective(objective_kw.get("loss"), objective_kw.get("regularizers"))
    z, c = np.linspace(1.0, 2.0, H.N, dtype=np.float32), (np.ones(H.N, np.float32) if weighted else None)
    opt = _bare(cls, objective, 0.375, white_background=True, **rgba_kw)
    loss = opt.accumulate(o, d, H.NEAR, far, target, n_total=H.N_TOTAL, depth=z, depth_weight=c, **extra)
    assert loss.dtype == torch.float64 and lib.names == [stem + "_depth"]
    name, a = lib.calls[0]
    assert len(a) == len(_lib.SIGNATURES[name][1]) == 19 and a[H.TERMS] and a[H.N_RAYS] == H.N and a[H.N_NORM] == H.N_TOTAL
    assert (a[H.OBJECTIVE] is None) == (objective is None) and (a[H.RGBA] is None) == (route != "_rgba")
    rec = a[DEPTH]
    assert rec["target"] and (rec["weight"] is not None) == weighted and rec["depth"] == 0.375
    assert tuple(opt.objective_terms()) == TERM_NAMES + ("opacity", "depth")
    # no rays: no launch, the terms are there and zero
    lib.calls.clear()
    loss = opt.accumulate(*H.rays(0)[:2], H.NEAR, H.rays(0)[2], np.zeros((0, columns), np.float32), depth=np.zeros(0, np.float32),
                          **(dict(background=np.zeros((0, 3), np.float32)) if per_call else {}))
    assert lib.calls == [] and float(loss) == 0.0 and float(opt.objective_terms()["depth"]) == 0.0


@pytest.mark.parametrize("cls,stem,tv,apply", H.CLASSES)
def test_depth_through_train_step_and_fit(lib, cls, stem, tv, apply):
    o, d, far = H.rays()
    target = np.full((H.N, 3), 0.5, np.float32)
    z = np.linspace(1.0, 2.0, H.N, dtype=np.float32)
    opt = _bare(cls, depth_loss=0.5)
    with pytest.raises(ValueError, match="depth_loss > 0 needs depth"):
        opt.train_step(o, d, H.NEAR, far, target)
    for bad in (dict(depth=z[:3]), dict(depth=z, depth_weight=z[:3]), dict(depth=z.reshape(H.N, 1))):
        with pytest.raises(ValueError, match="one value per ray"):
            opt.accumulate(o, d, H.NEAR, far, target, **bad)
    assert lib.calls == [] and opt.iterations == 0
    opt.train_step(o, d, H.NEAR, far, target, depth=z)
    assert lib.names == [stem + "_depth", apply]

    class Batches:                                                         # last_depth is set when a batch is drawn, as RayBatchDataset does
        last_depth = None

        def __iter__(self):
            for k in range(3):
                self.last_depth = (torch.as_tensor(z + k), None)
                yield target, (o, d, None)

    lib.calls.clear()
    out = opt.fit(Batches(), H.NEAR, far)
    assert list(out) == ["loss"] + list(TERM_NAMES) + ["opacity", "depth"] and all(len(v) == 3 for v in out.values())
    assert [n for n in lib.names if "rays" in n] == [stem + "_depth"] * 3
    # depth_loss = 0: the batches' depth is ignored and fit returns what it returned
    lib.calls.clear()
    out = _bare(cls).fit(Batches(), H.NEAR, far)
    assert list(out) == ["loss"] and [n for n in lib.names if "rays" in n] == [stem] * 3


def test_stage_batches_keep_last_depth_readable():
    class Source:
        last_depth = None

        def __iter__(self):
            for k in range(5):
                self.last_depth = k
                yield k

    src = Source()
    it = iter(src)
    for want in ([0, 1], [2, 3, 4]):
        stage = baked_train.StageBatches(src, it, len(want))
        got = [(k, stage.last_depth) for k in stage]
        assert got == [(k, k) for k in want]
    assert baked_train.StageBatches([1, 2], iter([1, 2]), 2).last_depth is None


# ---- RayBatchDataset.set_depth
def _dataset(views=3, rows=6, cols=8, budget=64.0):
    from keras_nerf_amd.data.raybatch import RayBatchDataset
    images = types.SimpleNamespace(image_loader=types.SimpleNamespace(output_size=(rows, cols)), image_paths=["x"] * views,
                                   device_cache_gb=budget)
    return RayBatchDataset(images, 16)


def test_set_depth_checks_shapes_and_the_budget():
    ds = _dataset()
    assert ds.last_depth is None and ds._depth is None
    good = np.zeros((3, 6, 8), np.float32)
    for bad in (np.zeros((3, 8, 6), np.float32), np.zeros((2, 6, 8), np.float32), np.zeros((3, 6, 8, 1), np.float32), np.zeros((144,), np.float32)):
        with pytest.raises(ValueError, match=r"depth must be \[3, 6, 8\]"):
            ds.set_depth(bad)
        with pytest.raises(ValueError, match=r"weight must be \[3, 6, 8\]"):
            ds.set_depth(good, bad)
    with pytest.raises(ValueError, match="weight without depth"):
        ds.set_depth(None, good)
    ds.set_depth(None)
    assert ds._depth is None and ds.last_depth is None
    # the maps count against device_cache_gb beside the images: 144 pixels x (16 + 8) bytes
    tight = _dataset(budget=144 * 20 / 1e9)
    with pytest.raises(ValueError, match="device_cache_gb"):
        tight.set_depth(good, good)
    with pytest.raises(ValueError, match="device_cache_gb"):
        _dataset(budget=144 * 18 / 1e9).set_depth(good)


def test_sparse_depth_needs_a_loaded_model_with_points(tmp_path):
    from keras_nerf_amd.data.colmap import ColmapDatasetLoader, read_points
    from tests.test_cameras_host import _write_colmap
    images = [f"{i + 1} 1 0 0 0 0 0 0 1 img_{i}.png" for i in range(3)]
    root = _write_colmap(tmp_path / "a", ["1 PINHOLE 8 6 7 7 4 3"], images)
    ld = ColmapDatasetLoader(root, holdout=2)
    with pytest.raises(ValueError, match="load_dataset"):
        ld.sparse_depth()
    ld.load_dataset(1, 8, 6, 0.5, 6.0, 4)
    with pytest.raises(ValueError, match="points3D.txt"):
        ld.sparse_depth("train")
    with pytest.raises(ValueError, match="subset"):
        ld.sparse_depth("all")
    points = ["7 0.1 0.2 4.0 10 20 30 0.75 1 0 2 5 3 1", "9 -0.1 0.0 3.0 1 2 3 1.5 2 0"]
    root = _write_colmap(tmp_path / "b", ["1 PINHOLE 8 6 7 7 4 3"], images, points)
    xyz, err, tracks = read_points(str(tmp_path / "b" / "sparse" / "0" / "points3D.txt"))
    assert xyz.dtype == np.float64 and np.array_equal(xyz, [[0.1, 0.2, 4.0], [-0.1, 0.0, 3.0]]) and np.array_equal(err, [0.75, 1.5])
    assert [t.tolist() for t in tracks] == [[1, 2, 3], [2]]
    scaled = ColmapDatasetLoader(root, holdout=2, bd_factor=0.75)
    scaled.load_dataset(1, 8, 6, 0.5, 6.0, 4)
    assert scaled.image_ids == [1, 2, 3] and np.isclose(scaled.scale, 1.0 / (scaled.bounds.min() / scaled.scale * 0.75))
    assert ColmapDatasetLoader(root, holdout=2).scale == 1.0


# ---- unit conversions
def test_ray_parameters_from_z_depth_and_distance():
    from keras_nerf_amd.data.depth import point_weights, ray_parameter_from_distance, ray_parameter_from_z
    rng = np.random.default_rng(0)
    # a camera somewhere: an orthonormal frame (right, up, backwards) and a centre
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = q, rng.standard_normal(3)
    # pinhole directions as the plain ray kernels write them: (x, -y, -1) in the camera's frame, not normalised
    xy = rng.uniform(-0.6, 0.6, (5, 7, 2))
    d = np.einsum("ij,hwj->hwi", q, np.stack([xy[..., 0], -xy[..., 1], -np.ones((5, 7))], axis=-1))
    t = rng.uniform(0.5, 6.0, (5, 7))
    pts = c2w[:3, 3] + t[..., None] * d
    z = -np.einsum("hwi,i->hw", pts - c2w[:3, 3], q[:, 2])                 # the depth along the viewing axis
    dist = np.linalg.norm(pts - c2w[:3, 3], axis=-1)
    assert np.allclose(z, t, rtol=1e-12)                                   # d_z = -1: for these rays z-depth IS the parameter
    assert np.allclose(ray_parameter_from_z(z, d, c2w), t, rtol=1e-12)
    assert np.allclose(ray_parameter_from_distance(dist, d), t, rtol=1e-12)
    # scaled and normalised directions: the parameter scales inversely
    for s in (0.25, 3.0):
        assert np.allclose(ray_parameter_from_z(z, d * s, c2w), t / s, rtol=1e-12)
        assert np.allclose(ray_parameter_from_distance(dist, d * s), t / s, rtol=1e-12)
    unit = d / np.linalg.norm(d, axis=-1, keepdims=True)
    assert np.allclose(ray_parameter_from_distance(dist, unit), dist, rtol=1e-12)
    assert np.allclose(ray_parameter_from_z(z, unit, c2w), dist, rtol=1e-12)
    # [V,4,4] with [V,H,W] maps, and torch tensors
    both = ray_parameter_from_z(np.stack([z, z]), np.stack([d, 2 * d]), np.stack([c2w, c2w]))
    assert np.allclose(both[0], t, rtol=1e-12) and np.allclose(both[1], t / 2, rtol=1e-12)
    got = ray_parameter_from_z(torch.as_tensor(z), torch.as_tensor(d), torch.as_tensor(c2w))
    assert isinstance(got, torch.Tensor) and np.allclose(got.numpy(), t, rtol=1e-12)
    got = ray_parameter_from_distance(torch.as_tensor(dist), torch.as_tensor(d))
    assert isinstance(got, torch.Tensor) and np.allclose(got.numpy(), t, rtol=1e-12)
    for bad in (lambda: ray_parameter_from_z(z, d[:4], c2w), lambda: ray_parameter_from_z(z, d, c2w[:3]),
                lambda: ray_parameter_from_z(z, d, np.stack([c2w] * 3)), lambda: ray_parameter_from_distance(dist, d[..., :2])):
        with pytest.raises(ValueError):
            bad()
    e = np.array([0.5, 1.0, 1.5])
    assert np.allclose(point_weights(e), np.exp(-(e / 1.0) ** 2)) and np.array_equal(point_weights([0.0, 0.0]), [1.0, 1.0])
    for bad in ([], [-1.0], [np.nan]):
        with pytest.raises(ValueError):
            point_weights(bad)
