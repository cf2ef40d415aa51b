"""Point queries, density grids and meshes of baked fields on the GPU (keras_nerf_amd/baked_query.py, csrc/baked_query.hip) against
the fp64 restatement tests/baked_query_reference.py, for dense, brick and 8-bit brick storage.  tests/README_baked_query.md states the
bound and counts its roundings."""
import functools

import numpy as np
import pytest

import baked_query_reference as R

pytestmark = pytest.mark.gpu

RES, LO, HI = (5, 6, 7), (-1.0, -0.5, 0.25), (1.5, 0.75, 2.0)          # distinct sizes, no multiple of either brick edge
SIZES = (1, 63, 64, 65, 257)                                            # wave, block and lane-group tails
STORAGES = ("dense", "brick4", "brick8", "quant4", "quant8")


def lanes_of(field):
    from keras_nerf_amd import baked_query
    return baked_query._storage(field)[1]


@functools.lru_cache(maxsize=None)
def fields(degree):
    """the three storages (bricks of both edges) of one random field on the 5 x 6 x 7 lattice, sigma zeroed in one octant so that at
    b = 4 a brick is absent; and the NumPy arrays they hold"""
    from keras_nerf_amd.baked import BakedField
    rng = np.random.default_rng(100 + degree)
    sigma = rng.uniform(0.5, 4.0, RES).astype(np.float32)
    sigma[3:, 3:, 3:] = 0.0
    co = rng.normal(0.0, 0.6, RES + ((degree + 1) ** 2, 3)).astype(np.float16)
    co[3:, 3:, 3:] = 0.0                                   # (so that the dense field holds what the bricks hold: zeros in the absent brick)
    dense = BakedField.from_arrays(sigma, co, (LO, HI))
    out = {"dense": dense, "brick4": dense.compact(4), "brick8": dense.compact(8)}
    out["quant4"], out["quant8"] = out["brick4"].quantize(), out["brick8"].quantize()
    assert int((out["brick4"].brick_of < 0).sum()) >= 1 and int((out["brick8"].brick_of < 0).sum()) == 0
    return out, sigma, co


@functools.lru_cache(maxsize=None)
def stored_arrays(degree, name):
    """(sigma, coefficients) the reference is fed for a storage: the dense arrays of what the storage holds.  A brick field has zeros
    where a brick is absent; a quantised one holds the decoded coefficients"""
    f = fields(degree)[0][name]
    d = f if name == "dense" else f.to_dense()
    return d.sigma.cpu().numpy(), d.coefficients.cpu().numpy()


@functools.lru_cache(maxsize=None)
def point_set(n):
    """n points: an interior one, points exactly on lo and hi faces (u = cells), on interior cell faces, outside on each side, one NaN
    coordinate, then random interior points.  (float32 [n,3], outside bool [n])"""
    rng = np.random.default_rng(n)
    lo, hi = np.asarray(LO, dtype=np.float32), np.asarray(HI, dtype=np.float32)
    mid = (lo + hi) / 2
    cell = (hi - lo) / (np.asarray(RES, dtype=np.float32) - 1)          # 0.625 and 0.25 are exact
    special = [mid + cell * 0.3,
               [lo[0], mid[1], mid[2]], [mid[0], lo[1], mid[2]], [mid[0], mid[1], lo[2]], lo,
               [hi[0], mid[1], mid[2]], [mid[0], hi[1], mid[2]], [mid[0], mid[1], hi[2]], hi,
               [lo[0] + 2 * cell[0], mid[1], mid[2]], [mid[0], lo[1] + 3 * cell[1], mid[2]], lo + cell, [lo[0] + 3 * cell[0], lo[1] + 4 * cell[1], mid[2]],
               [lo[0] - 0.01, mid[1], mid[2]], [hi[0] + 0.01, mid[1], mid[2]], [mid[0], lo[1] - 1.0, mid[2]], [mid[0], hi[1] + 1e-3, mid[2]],
               [mid[0], mid[1], lo[2] - 1e-3], [mid[0], mid[1], hi[2] + 5.0], [mid[0], np.nan, mid[2]]]
    special = np.asarray(special, dtype=np.float32)
    outside = np.zeros(len(special), dtype=bool)
    outside[13:] = True
    rest = rng.uniform(lo, hi, (max(0, n - len(special)), 3)).astype(np.float32)
    return np.concatenate([special, rest])[:n].copy(), np.concatenate([outside, np.zeros(len(rest), dtype=bool)])[:n]


def direction_modes(n):
    rng = np.random.default_rng(7 * n)
    per = (rng.normal(size=(n, 3)) * rng.uniform(0.1, 30.0, (n, 1))).astype(np.float32)        # not unit vectors
    per[min(5, n - 1)] = 0.0                                                                   # one zero-length row
    return {"none": None, "shared": np.array([0.3, -2.0, 1.1], dtype=np.float32), "per point": per}


def check(got, ref, output, degree, what):
    """|GPU - reference| <= 2 x roundings x 2^-24 x the sum of the absolute values of the output's terms"""
    g = got.detach().cpu().numpy().astype(np.float64).reshape(ref[output].shape)
    err, bnd = np.abs(g - ref[output]), R.bound(output, ref[output + "_abs"], degree)
    bad = err > bnd
    assert not bad.any(), f"{what} {output}: {int(bad.sum())} values past the bound, worst error {err[bad].max():.3g} against {bnd[bad].min():.3g}"


def same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_query_against_the_reference_and_across_storages(degree):
    """checks 1, 3, 4 and 7: every storage and lane variant against fp64; dense and bricks bit-identical; the 8-bit records at one lane
    the bits of the brick query on the dequantised records; the sigma-only path the bits of the full path; zeros outside"""
    import torch
    from keras_nerf_amd import baked_query
    F = fields(degree)[0]
    deq = {b: F[f"quant{b}"].dequantize() for b in (4, 8)}
    for n in SIZES:
        pts, outside = point_set(n)
        for mode, d in direction_modes(n).items():
            ref = {name: R.query(*stored_arrays(degree, name), LO, HI, pts, d) for name in ("dense", "quant4", "quant8")}
            ref["brick4"] = ref["brick8"] = ref["dense"]             # (the absent brick's records are zero in the dense field too)
            got = {}
            for name in STORAGES:
                for lanes in lanes_of(F[name]):
                    what = f"degree {degree} {name} lanes {lanes} n {n} directions {mode}"
                    rgb, sigma, grad = got[name, lanes] = F[name].query(pts, d, gradient=True, lanes_per_point=lanes)
                    assert rgb.shape == (n, 3) and sigma.shape == (n, 1) and grad.shape == (n, 3), what
                    check(sigma, ref[name], "sigma", degree, what)
                    check(rgb.reshape(-1, 3), ref[name], "rgb", degree, what)
                    check(grad, ref[name], "grad", degree, what)
                    o = torch.as_tensor(outside, device=rgb.device)
                    assert not rgb[o].any() and not sigma[o].any() and not grad[o].any(), what
                    assert bool(torch.isfinite(rgb).all() and torch.isfinite(sigma).all() and torch.isfinite(grad).all()), what
            for lanes in lanes_of(F["dense"]):
                assert same(got["dense", lanes], got["brick8", lanes]), (degree, lanes, n, mode)
                assert same(got["dense", lanes], got["brick4", lanes]), (degree, lanes, n, mode)
            for b in (4, 8):
                assert same(got[f"quant{b}", 1], deq[b].query(pts, d, gradient=True, lanes_per_point=1)), (degree, b, n, mode)
        for name in STORAGES:
            s, g = baked_query.query_sigma(F[name], pts, gradient=True)
            for lanes in lanes_of(F[name]):
                assert same((s, g), got[name, lanes][1:]), (degree, name, lanes, n)
            assert torch.equal(baked_query.query_sigma(F[name], pts), s)


def test_lattice_points_return_the_stored_sigma_bit_for_bit():
    """check 2: box [-1, 1]^3, R = 5 (cell 0.5, scale 2, every step exact), points at multiples of 0.5"""
    import torch
    from keras_nerf_amd import baked_query
    from keras_nerf_amd.baked import BakedField
    rng = np.random.default_rng(5)
    sigma = rng.uniform(0.1, 9.0, (5, 5, 5)).astype(np.float32)
    co = rng.normal(0.0, 0.6, (5, 5, 5, 4, 3)).astype(np.float16)
    dense = BakedField.from_arrays(sigma, co, ((-1.0,) * 3, (1.0,) * 3))
    idx = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), axis=-1).reshape(5, 5, 5, 3)
    pts = (idx * 0.5 - 1.0).astype(np.float32)
    want = torch.as_tensor(sigma).to(dense.device)
    y0 = np.float32(0.28209479177387814)
    for f in (dense, dense.compact(4), dense.compact(4).quantize()):
        for lanes in lanes_of(f):
            rgb, sg = f.query(pts, lanes_per_point=lanes)
            assert sg.shape == (5, 5, 5, 1) and torch.equal(sg[..., 0], want)
        assert torch.equal(baked_query.query_sigma(f, pts)[..., 0], want)
        assert torch.equal(f.density_grid((5, 5, 5), ((-1.0,) * 3, (1.0,) * 3)), want)          # grid mode forms the same points
    # at a lattice point one weight is 1 and seven are 0: the DC colour is one product (the unquantised storages hold co as it is)
    rgb = dense.query(pts)[0].cpu().numpy()
    assert np.array_equal(rgb, np.clip(co[..., 0, :].astype(np.float32) * y0, 0.0, 1.0))


@pytest.mark.parametrize("degree", [0, 2, 3])
def test_grid_mode_equals_point_mode(degree):
    """check 5, on a grid whose box is not the field's (part of it lies outside), with distinct sizes per axis"""
    import torch
    from keras_nerf_amd import baked_query
    F = fields(degree)[0]
    res, lo, hi = (4, 3, 5), (-1.2, -0.6, 0.2), (1.6, 0.7, 1.9)
    pts = R.grid_points(res, lo, hi).reshape(res + (3,))
    d = np.array([0.2, 0.5, -1.0], dtype=np.float32)
    for name in STORAGES:
        f = F[name]
        for lanes in lanes_of(f):
            rgb, sigma, grad = f.query(pts, d, gradient=True, lanes_per_point=lanes)
            gs, gc, gg = baked_query.query_grid(f, res, lo, hi, d, gradient=True, lanes_per_point=lanes)
            assert torch.equal(gs, sigma[..., 0]) and torch.equal(gc, rgb) and torch.equal(gg, grad), (degree, name, lanes)
        sg, col = f.density_grid(res, (lo, hi), direction=d)
        assert torch.equal(sg, f.density_grid(res, (lo, hi))) and torch.equal(sg, gs)
        assert torch.equal(col, f.query(pts, d)[0])
        assert bool((sg == 0).any()) and bool((sg > 0).any())       # the grid does reach past the box


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_density_grid_without_arguments_is_the_stored_column(degree):
    """check 6"""
    import torch
    F = fields(degree)[0]
    for name in STORAGES:
        f = F[name]
        want = (f if name == "dense" else f.to_dense()).sigma
        got = f.density_grid()
        assert got.shape == RES and got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, want), (degree, name)
        sg, col = f.density_grid(direction=[0.0, 0.0, 1.0])
        assert torch.equal(sg, want) and col.shape == RES + (3,)
        assert torch.equal(col, f.query(R.grid_points(RES, LO, HI).reshape(RES + (3,)), [0.0, 0.0, 1.0])[0])


def test_a_brick_table_entry_out_of_range_reads_as_absent():
    """check 7: the existing guard (slot >= 0 && slot < n_bricks), exercised on valid memory: no record past the table is read"""
    from keras_nerf_amd.baked import BrickBakedField
    from keras_nerf_amd.baked_quant import QuantizedBrickField
    F = fields(2)[0]
    pts, _ = point_set(257)
    d = direction_modes(257)["per point"]
    for name in ("brick4", "quant4"):
        f = F[name]
        tables = []
        for value in (f.n_bricks, -1):
            t = f.brick_of.clone()
            t[0, 1, 0] = value
            tables.append(t.contiguous())
        if name == "brick4":
            a, b = (BrickBakedField(f._records, t, f._words, f.resolution, f.bounds, f.sh_degree, f.brick) for t in tables)
        else:
            a, b = (QuantizedBrickField(f._records, f._exponents, t, f._words, f.resolution, f.bounds, f.sh_degree, f.brick) for t in tables)
        for lanes in lanes_of(f):
            out = a.query(pts, d, gradient=True, lanes_per_point=lanes)
            assert same(out, b.query(pts, d, gradient=True, lanes_per_point=lanes))
            assert not same(out, f.query(pts, d, gradient=True, lanes_per_point=lanes))       # the brick did matter


def test_extract_mesh_is_marching_cubes_on_the_density_grid():
    """check 8"""
    from keras_nerf_amd.runtime import marching_cubes
    F = fields(1)[0]
    for name in STORAGES:
        f = F[name]
        for res, bounds in ((None, None), ((9, 8, 11), ((-1.2, -0.6, 0.2), (1.6, 0.7, 1.9)))):
            lo, hi = bounds if bounds else f.bounds
            mesh = f.extract_mesh(2.0, res, bounds)
            want = marching_cubes(f.density_grid(res, bounds), 2.0, lo, hi)
            assert len(mesh) == 3 and mesh[0].shape[0] > 0 and mesh[1].shape[0] > 0 and same(mesh, want), (name, res)
        empty = f.extract_mesh(1e9, vertex_colors=True)
        assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 3), (0, 3), (0, 3)]


def test_a_sphere_meshes_closed_near_the_analytic_surface():
    """check 9: sigma = max(0, r0 - |x|) k on 17^3"""
    import torch
    from keras_nerf_amd.baked import BakedField
    r0, k, thr, R17 = 0.7, 10.0, 2.0, 17
    ax = np.linspace(-1.0, 1.0, R17)
    x = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1)
    sigma = (np.maximum(0.0, r0 - np.linalg.norm(x, axis=-1)) * k).astype(np.float32)
    co = np.random.default_rng(9).normal(0.0, 0.6, (R17,) * 3 + (4, 3)).astype(np.float16)
    dense = BakedField.from_arrays(sigma, co, ((-1.0,) * 3, (1.0,) * 3))
    diagonal = np.sqrt(3.0) * 2.0 / (R17 - 1)
    for f in (dense, dense.compact(8), dense.compact(4).quantize()):
        verts, faces, normals, colors = f.extract_mesh(thr, vertex_colors=True)
        v, t = verts.cpu().numpy().astype(np.float64), faces.cpu().numpy().astype(np.int64)
        assert len(v) > 100 and len(t) > 200
        edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
        _, counts = np.unique(edges, axis=0, return_counts=True)
        assert (counts == 2).all()                                  # closed: every edge is in exactly two faces
        assert np.abs(np.linalg.norm(v, axis=1) - (r0 - thr / k)).max() <= diagonal
        assert torch.equal(colors, f.query(verts, -normals)[0]) and colors.shape == verts.shape
        assert bool((colors > 0).any())


@pytest.mark.parametrize("storage", ["dense", "brick"])
def test_the_live_field_of_an_optimiser_answers_queries(storage):
    """check 10: opt.field is one of these classes already: after a train step its query is the query of opt.finish().  (sigma stays
    above 0 at every stored point after one small step, so finish() keeps every brick and changes no record)"""
    from keras_nerf_amd.baked_train import brick_optimizer
    F = fields(2)[0]
    src = F["dense"] if storage == "dense" else F["brick4"]
    opt = src.optimizer(1e-3, 1e-3) if storage == "dense" else brick_optimizer(src, 1e-3, 1e-3)
    rng = np.random.default_rng(3)
    n = 64
    o = np.concatenate([rng.uniform(LO, HI, (n, 3))[:, :2], np.full((n, 1), -1.0)], axis=1).astype(np.float32)
    d = np.tile(np.array([[0.02, -0.01, 1.0]], dtype=np.float32), (n, 1))
    opt.train_step(o, d, 0.5, 3.5, rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32))
    pts, _ = point_set(257)
    dirs = direction_modes(257)["per point"]
    live = opt.field.query(pts, dirs, gradient=True)
    assert same(live, opt.finish().query(pts, dirs, gradient=True))
    assert not same(live, src.query(pts, dirs, gradient=True))      # the step did change the field
    assert same((opt.field.density_grid(),), (opt.finish().density_grid(),))
    mesh = opt.field.extract_mesh(2.0, vertex_colors=True)
    assert mesh[0].shape[0] > 0 and same(mesh, opt.finish().extract_mesh(2.0, vertex_colors=True))
