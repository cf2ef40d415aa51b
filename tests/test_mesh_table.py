"""The marching-cubes table (keras_nerf_amd/mesh_table.py -> csrc/mesh_table.h) and the NumPy reference of csrc/mesh.hip on analytic
fields, plus the PLY writer (CPU)."""
import itertools
import os

import numpy as np
import pytest

from keras_nerf_amd import mesh_table as MT
from tests import mc_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_header_is_the_generators_output():
    assert open(MT.HEADER).read() == MT.render()


def _crossed(case):
    return {i for i, (c0, c1, _) in enumerate(MT.EDGES) if ((case >> c0) & 1) != ((case >> c1) & 1)}


@pytest.mark.parametrize("case", range(256))
def test_every_case_uses_exactly_its_crossed_edges(case):
    tris = MT.case_triangles(case)
    assert {e for t in tris for e in t} == _crossed(case)
    assert all(len(set(t)) == 3 for t in tris)


def _boundary(case):
    """directed edges of the case's triangles that are not cancelled by their reverse inside the cube"""
    de = [(t[i], t[(i + 1) % 3]) for t in MT.case_triangles(case) for i in range(3)]
    s = set(de)
    assert len(s) == len(de)
    return {e for e in de if (e[1], e[0]) not in s}


def _mirror_edge(i, a):
    """cube edge i on face (a, 1) of one cube -> the same grid edge as an edge of face (a, 0) of the neighbour along +a"""
    c0, c1, ax = MT.EDGES[i]
    m0, m1 = c0 & ~(1 << a), c1 & ~(1 << a)
    return next(j for j, (d0, d1, ay) in enumerate(MT.EDGES) if (d0, d1, ay) == (m0, m1, ax))


def test_neighbours_contribute_the_same_face_segments_in_reverse():
    """for each face configuration (4 corner bits) and every pair of cases that share it, the boundary segments cube A has on its +a
    face are those the neighbour B has on its -a face, reversed"""
    bnd = [_boundary(c) for c in range(256)]
    for a in range(3):
        hi_c = [c for c in range(8) if (c >> a) & 1]
        fe_hi = set(MT.face_edges(MT.FACES.index((a, 1))))
        fe_lo = set(MT.face_edges(MT.FACES.index((a, 0))))
        for ca, cb in itertools.product(range(256), range(256)):
            if any(((ca >> c) & 1) != ((cb >> (c & ~(1 << a))) & 1) for c in hi_c):
                continue
            sa = {(_mirror_edge(p, a), _mirror_edge(q, a)) for p, q in bnd[ca] if p in fe_hi and q in fe_hi}
            sb = {(q, p) for p, q in bnd[cb] if p in fe_lo and q in fe_lo}
            assert sa == sb, (a, ca, cb)


def test_sphere_is_a_closed_genus_0_surface_with_the_analytic_volume():
    res, r = 128, 1.0
    v, f, n = M.marching_cubes(M.sphere(res, r), 0.0, (-1.5,) * 3, (1.5,) * 3)
    M.check_closed_manifold(f, len(v))
    assert M.euler(f, len(v)) == 2
    vol = M.signed_volume(v, f)
    assert vol > 0 and abs(vol - 4 / 3 * np.pi * r ** 3) < 0.01 * (4 / 3 * np.pi * r ** 3), vol
    # normals point outward (toward lower density): radially
    assert (np.einsum("ij,ij->i", n, v / np.linalg.norm(v, axis=1, keepdims=True)) > 0.99).all()


def test_torus_has_euler_characteristic_0():
    v, f, _ = M.marching_cubes(M.torus(96), 0.0, (-1.5,) * 3, (1.5,) * 3)
    M.check_closed_manifold(f, len(v))
    assert M.euler(f, len(v)) == 0
    assert M.signed_volume(v, f) > 0


def test_two_spheres_have_euler_characteristic_4():
    s = np.maximum(M.sphere(64, 0.5, (-0.7, 0, 0)), M.sphere(64, 0.5, (0.7, 0.1, 0)))
    v, f, _ = M.marching_cubes(s, 0.0, (-1.5,) * 3, (1.5,) * 3)
    M.check_closed_manifold(f, len(v))
    assert M.euler(f, len(v)) == 4


def test_grid_values_exactly_at_the_threshold():
    """sigma == tau is outside: vertices then sit exactly on grid points, indices stay distinct, the mesh stays closed"""
    s = np.round(M.sphere(40, 1.0) * 8).astype(np.float32) / 8       # many points exactly 0
    assert (s == 0).sum() > 100
    v, f, _ = M.marching_cubes(s, 0.0, (-1.5,) * 3, (1.5,) * 3)
    M.check_closed_manifold(f, len(v))
    assert M.euler(f, len(v)) == 2


def test_random_fields_give_closed_oriented_manifolds():
    """ambiguous faces everywhere: a random field, zero on the border (the surface does not reach it)"""
    rng = np.random.default_rng(3)
    s = rng.standard_normal((20, 18, 22)).astype(np.float32)
    s[0], s[-1], s[:, 0], s[:, -1], s[:, :, 0], s[:, :, -1] = -1, -1, -1, -1, -1, -1
    v, f, _ = M.marching_cubes(s, 0.0, (-1,) * 3, (1,) * 3)
    M.check_closed_manifold(f, len(v))


def _read_ply(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elems, cur = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[0] == "element":
            cur = [w[1], int(w[2]), []]; elems.append(cur)
        elif w[0] == "property":
            cur[2].append(w[1:])
    tmap = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    out, off = {}, 0
    for name, count, props in elems:
        if props[0][0] == "list":
            dt = np.dtype([("n", tmap[props[0][1]]), ("i", tmap[props[0][2]], (3,))])
        else:
            dt = np.dtype([(p[1], tmap[p[0]]) for p in props])
        out[name] = np.frombuffer(body, dt, count, off)
        off += dt.itemsize * count
    assert off == len(body)
    return out


def test_save_ply_round_trips(tmp_path):
    from keras_nerf_amd.io.ply import save_ply
    rng = np.random.default_rng(0)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    n = rng.standard_normal((7, 3)).astype(np.float32)
    c = rng.random((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, (5, 3)).astype(np.int32)
    p = str(tmp_path / "m.ply")
    save_ply(p, v, f, normals=n, colors=c)
    r = _read_ply(p)
    got_v = np.stack([r["vertex"][k] for k in "xyz"], 1)
    got_n = np.stack([r["vertex"][k] for k in ("nx", "ny", "nz")], 1)
    got_c = np.stack([r["vertex"][k] for k in ("red", "green", "blue")], 1)
    assert np.array_equal(got_v, v) and np.array_equal(got_n, n)
    assert np.array_equal(got_c, np.rint(c * 255).astype(np.uint8))
    assert (r["face"]["n"] == 3).all() and np.array_equal(r["face"]["i"], f)
    save_ply(p, v, f)                                   # positions and faces only
    r = _read_ply(p)
    assert r["vertex"].dtype.names == ("x", "y", "z") and np.array_equal(r["face"]["i"], f)
    save_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))      # an empty surface is a valid file
    r = _read_ply(p)
    assert len(r["vertex"]) == 0 and len(r["face"]) == 0
