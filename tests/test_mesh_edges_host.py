"""What tests/test_gpu_mesh_edges.py rests on, without a device: the float64 form of the marching-cubes reference, the case table
`mc_reference.EDGE_GRIDS` (scan block counts, cube-case coverage, normal exclusions) and four reference mutants that the table has
to be able to see."""
import numpy as np
import pytest

from tests import mc_reference as M

LO, HI = (-1.5,) * 3, (1.5,) * 3
EXT = 3.0
f32, f64 = np.float32, np.float64
SMALL = [k for k in M.EDGE_GRIDS if k not in M.LARGE_GRIDS]


@pytest.fixture(scope="module")
def results():
    """name -> (grid, tau, float32 mirror, float64 form, details), computed once and left unchanged"""
    out = {}
    for name in SMALL:
        make, tau = M.EDGE_GRIDS[name]
        g = make()
        (r32, r64), det = M.marching_cubes(g, tau, LO, HI, dtype=(f32, f64), details=True)
        out[name] = (g, tau, r32, r64, det)
    return out


def test_float64_form_is_a_closed_sphere_with_the_analytic_volume():
    """as test_mesh_table.py asks of the float32 form; and the two forms share their faces and differ by float32 rounding only"""
    res, r = 128, 1.0
    (v32, f_32, n32), (v, f, n) = M.marching_cubes(M.sphere(res, r), 0.0, LO, HI, dtype=(f32, f64))
    assert v.dtype == f64 and n.dtype == f64 and np.array_equal(f, f_32)
    M.check_closed_manifold(f, len(v))
    assert M.euler(f, len(v)) == 2
    vol = M.signed_volume(v, f)
    assert vol > 0 and abs(vol - 4 / 3 * np.pi * r ** 3) < 0.01 * (4 / 3 * np.pi * r ** 3), vol
    assert (np.einsum("ij,ij->i", n, v / np.linalg.norm(v, axis=1, keepdims=True)) > 0.99).all()
    assert np.abs(v32 - v).max() < 1e-6 * EXT and np.abs(n32 - n).max() < 1e-4


def test_default_dtype_is_the_float32_mirror():
    g = M.noise((6, 7, 5), 1)
    v, f, n = M.marching_cubes(g, 0.0, LO, HI)
    ((v2, f2, n2),) = M.marching_cubes(g, 0.0, LO, HI, dtype=(f32,))
    assert v.dtype == f32 and n.dtype == f32 and np.array_equal(v, v2) and np.array_equal(f, f2) and np.array_equal(n, n2)


def test_scan_block_counts_of_the_table():
    """what the grids promise about the device's multi-level scan (blocks of M.SCAN_BLOCK elements per level)"""
    def levels(n):
        out = []
        while True:
            n = -(-n // M.SCAN_BLOCK)
            out.append(n)
            if n == 1:
                return out
    size = lambda name: int(np.prod(M.EDGE_GRIDS[name][0]().shape)) if name not in M.LARGE_GRIDS else \
        {"noise_71": 71 ** 3, "noise_1025x32x32": 1025 * 32 * 32}[name]
    assert levels(size("one_corner")) == [1] and levels(3 * size("one_corner")) == [1]
    n = size("noise_5x5x41")
    assert n == 1025 and levels(n) == [2, 1] and levels(3 * n) == [4, 1] and n % M.SCAN_BLOCK == 1 and 3 * n % M.SCAN_BLOCK == 3
    n = size("noise_8x8x16")
    assert n == 1024 and levels(n) == [1] and levels(3 * n) == [3, 1]
    n = size("noise_71")
    assert 3 * n == 1_073_733 and levels(3 * n) == [1049, 2, 1] and 3 * n % M.SCAN_BLOCK and 1049 % M.SCAN_BLOCK
    n = size("noise_1025x32x32")
    assert n == 1_049_600 and levels(n) == [1025, 2, 1] and 1025 % M.SCAN_BLOCK == 1


def test_noise_17_covers_all_256_cases(results):
    """a change of seed cannot silently lose a table row"""
    cases = results["noise_17"][4]["cases"]
    assert np.unique(cases).size == 256
    g, tau, (v, f, n), _, _ = results["noise_17_padded"]
    M.check_closed_manifold(f, len(v))


def test_every_corner_pattern_is_its_own_table_row():
    from keras_nerf_amd import mesh_table as MT
    counts, _ = MT.table()
    for case in range(256):
        (v, f, n), det = M.marching_cubes(M.corner_pattern(case), 0.0, LO, HI, details=True)
        assert det["cases"].tolist() == [case] and len(f) == counts[case]


def test_what_the_special_grids_hold(results):
    g, tau, (v, f, n), (dv, _, dn), det = results["checkerboard_24x23x22"]
    crossable = sum(np.prod([r - (k == a) for k, r in enumerate(g.shape)]) for a in range(3))
    assert len(v) == crossable and len(v) > 0.95 * 3 * g.size                 # every edge that exists is crossed
    zero = (n == 0).all(1)
    assert zero.sum() > 0.9 * len(v) and np.array_equal(zero, (dn == 0).all(1))
    g, tau, (v, f, n), _, det = results["integers_20x21x22"]
    assert (g == tau).sum() > 1000
    e = det["edges"]
    t0 = g.reshape(-1)[e // 3] == tau                                         # crossed edges whose near end is on the threshold: t = 0
    assert t0.sum() > 1000
    assert len(np.unique(v, axis=0)) < len(v)                                 # coinciding vertices with distinct ids
    assert np.unique(f).size == len(v)
    for name in ("all_inside", "all_outside"):
        (v, f, n) = results[name][2]
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    assert results["one_corner"][2][0].shape == (3, 3) and results["one_corner"][2][1].shape == (1, 3)


@pytest.mark.parametrize("name", list(M.EDGE_GRIDS))
def test_normal_exclusions_stay_under_the_cap(name, results):
    if name in results:
        r64, det = results[name][3], results[name][4]
    else:
        make, tau = M.EDGE_GRIDS[name]
        r64, det = M.marching_cubes(make(), tau, LO, HI, dtype=f64, details=True)
    keep = M.comparable_normals(det["lengths"][-1])
    share = 1 - keep.mean() if keep.size else 0.0
    print(f"{name}: {keep.size} vertices, {share:.3%} of the normals not compared with float64")
    assert share <= M.NORMAL_CAP


def test_sphere_and_torus_exclude_no_normal():
    for g, tau in ((M.sphere(48), 0.0), (np.ascontiguousarray(M.torus(61)[:, :50, 3:]), 0.05)):
        _, det = M.marching_cubes(g, tau, LO, HI, dtype=f64, details=True)
        assert M.comparable_normals(det["lengths"][0]).all()


def _shows(ref32, ref64, det, mut):
    """does the mutant's result fail the checks tests/test_gpu_mesh_edges.py applies to a device result?"""
    (rv, rf, rn), (dv, _, dn) = ref32, ref64
    mv, mf, mn = mut
    if mf.shape != rf.shape or not np.array_equal(mf, rf) or mv.shape != rv.shape:
        return "faces"
    keep = M.comparable_normals(det["lengths"][1])
    tol_v, tol_n = M.float64_bounds(EXT, ref32, ref64, keep)
    if np.abs(mv - rv).max(initial=0) > 1e-6 * EXT or np.abs(mv - dv).max(initial=0) > tol_v:
        return "vertices"
    if np.abs(mn - rn).max(initial=0) > 1e-6 * EXT or np.abs(mn - dn)[keep].max(initial=0) > tol_n:
        return "normals"
    return None


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_table_sees_each_reference_mutant(mutant, results):
    seen = {}
    for name, (g, tau, r32, r64, det) in results.items():
        how = _shows(r32, r64, det, M.marching_cubes(g, tau, LO, HI, mutant=mutant))
        if how:
            seen[name] = how
    print(f"{mutant}: {seen}")
    assert seen, mutant
    expected = {"ge": "integers_20x21x22", "scan": "noise_5x5x41", "two_sided": "slab_2x64x64", "far_t": "noise_17"}[mutant]
    assert expected in seen
    if mutant == "scan":                                  # one block: nothing to drop
        assert "one_corner" not in seen and "noise_8x8x16" in seen      # three edge-scan blocks, though one cube-scan block
