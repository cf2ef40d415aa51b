"""csrc/mesh.hip at its limits: every grid of `mc_reference.EDGE_GRIDS` (scan levels with partial blocks, all 256 cube cases, samples on the
threshold, slabs, the densest output, empty surfaces) against the float32 mirror AND the float64 form of tests/mc_reference.py; the C
entry point's partial outputs, workspace reuse and refusals; locality of a non-finite sample.

Against the mirror: faces `array_equal`, vertices and normals within 1e-6 x extent (`test_gpu_mesh._same_as_reference`).  Against float64:
vertices within max(1e-6 x extent, 4 x the mirror's own largest deviation from float64 in that case); normals the same way, where the
float64 un-normalised gradient is longer than 1e-3 x the case's median or exactly zero (`mc_reference.comparable_normals`; at most 3 %
of a case may be left out, nothing on the sphere and the torus -- in fact nothing anywhere); a normal that is exactly zero in the mirror
is exactly zero on the device.

Measured on an MI355X (pytest -s prints them; not asserted): 0 of the vertices differ in bits from the float32 mirror in every case.
Of the normals 15.2 ... 15.6 % do on the noise grids (6 % on the integer grid, 0 on the checkerboard), each by one unit in the last
place of a component and far inside the bounds: the compiler's headers map `__fsqrt_rn` to the native square root (about 1 ulp)
unless OCML_BASIC_ROUNDED_OPERATIONS is defined, so the normal's length is not always the correctly rounded one NumPy divides by.
Every other `__f*_rn` operation of the kernel is the plain IEEE one, as the vertices show.  Worst errors against float64: vertices
3.2e-7 (bound 3e-6); normals 2.7e-5 beside a bound of 1.07e-4 on the 1025 x 32 x 32 grid, and everywhere at a quarter of the bound,
which is the mirror's own error, or below.  One normal of 1,540,365 is left out on that grid, none anywhere else."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mc_reference as M
from tests.test_gpu_mesh import EXT, HI, LO, _gpu_mc, _same_as_reference

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32)
    return float((a != b).any(1).mean()) if len(a) else 0.0


def _check(name, grid, tau, max_excluded=M.NORMAL_CAP):
    """the device's mesh of `grid` against both forms of the reference; returns the device arrays and the reference's details"""
    (r32, r64), det = M.marching_cubes(grid, tau, LO, HI, dtype=(f32, f64), details=True)
    v, f, n = _same_as_reference(grid, tau, ref=r32)
    assert v.shape == (len(r32[0]), 3) and f.shape == (len(r32[1]), 3) and n.shape == v.shape
    keep = M.comparable_normals(det["lengths"][1])
    assert (1 - keep.mean() if keep.size else 0.0) <= max_excluded
    tol_v, tol_n = M.float64_bounds(EXT, r32, r64, keep)
    ev = float(np.abs(v - r64[0]).max(initial=0))
    en = float(np.abs(n - r64[2])[keep].max(initial=0))
    zero = (r32[2] == 0).all(1)
    print(f"{name}: V {len(v)} F {len(f)}; vertices {ev:.2e} (bound {tol_v:.2e}), normals {en:.2e} (bound {tol_n:.2e}), "
          f"{int((~keep).sum())} normals left out, {int(zero.sum())} exactly zero; differ in bits from the mirror: "
          f"vertices {_bits_differ(v, r32[0]):.3%}, normals {_bits_differ(n, r32[2]):.3%}")
    assert ev <= tol_v and en <= tol_n
    assert (n[zero] == 0).all()
    return (v, f, n), (r32, r64, det)


@pytest.mark.parametrize("name", list(M.EDGE_GRIDS))
def test_edge_grid_matches_both_forms_of_the_reference(name):
    make, tau = M.EDGE_GRIDS[name]
    grid = make()
    (v, f, n), (r32, r64, det) = _check(name, grid, tau)
    if name == "one_corner":
        assert v.shape == (3, 3) and f.shape == (1, 3)
    if name == "noise_17":
        assert np.unique(det["cases"]).size == 256
    if name == "noise_17_padded":
        M.check_closed_manifold(f, len(v))
    if name == "checkerboard_24x23x22":
        assert (n == 0).all(1).sum() > 0.9 * len(v) and len(v) > 0.95 * 3 * grid.size
    if name == "integers_20x21x22":
        assert len(np.unique(v, axis=0)) < len(v) and np.unique(f).size == len(v)      # coinciding vertices keep distinct ids
    if name.startswith("all_"):
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    if name in M.LARGE_GRIDS:
        assert len(v) > 500_000 and len(f) > 1_000_000


def test_every_cube_case_on_its_own():
    """2x2x2 grids of +-1: each of the 256 table rows through face_emit_kernel alone, every normal from one-sided gradients"""
    from keras_nerf_amd import mesh_table as MT
    counts, _ = MT.table()
    for case in range(256):
        (v, f, n), (r32, r64, det) = _check(f"case {case}", M.corner_pattern(case), 0.0)
        assert det["cases"].tolist() == [case] and len(f) == counts[case]


def test_sphere_and_torus_leave_no_normal_out():
    _check("sphere 48", M.sphere(48), 0.0, max_excluded=0.0)
    _check("torus 61 sliced", np.ascontiguousarray(M.torus(61)[:, :50, 3:]), 0.05, max_excluded=0.0)


# ---- the C entry point itself

class _Raw:
    def __init__(self):
        from keras_nerf_amd import _lib
        self.lib, self.INVALID = _lib.load(), _lib.KNERF_ERR_INVALID
        self.lo, self.hi = (C.c_float * 3)(*LO), (C.c_float * 3)(*HI)

    def call(self, grid, shape, tau, ws, nbytes, counts, v=None, f=None, n=None):
        from keras_nerf_amd.runtime import _ptr
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return self.lib.knerf_marching_cubes(stream, _ptr(grid), *shape, self.lo, self.hi, float(tau), _ptr(ws), C.byref(nbytes), counts,
                                             _ptr(v), _ptr(f), _ptr(n))

    def size(self, shape):
        nbytes, counts = C.c_size_t(0), (C.c_int64 * 2)()
        rc = self.call(None, shape, 0.0, None, nbytes, counts)
        return rc, nbytes.value

    def count(self, grid, tau, ws):
        nbytes, counts = C.c_size_t(ws.numel()), (C.c_int64 * 2)()
        assert self.call(grid, grid.shape, tau, ws, nbytes, counts) == 0
        return nbytes, counts

    def emit(self, grid, tau, ws, nbytes, counts, which="vfn"):
        V, F = int(counts[0]), int(counts[1])
        out = {"v": torch.full((V, 3), -7.0, device="cuda"), "f": torch.full((F, 3), -7, device="cuda", dtype=torch.int32),
               "n": torch.full((V, 3), -7.0, device="cuda")}
        assert self.call(grid, grid.shape, tau, ws, nbytes, counts, *[out[k] if k in which else None for k in "vfn"]) == 0
        return {k: out[k].cpu().numpy() for k in which}


def test_emit_phase_with_a_subset_of_its_outputs():
    raw = _Raw()
    grid = torch.as_tensor(M.noise((17, 17, 17)), device="cuda")
    rc, need = raw.size(grid.shape)
    assert rc == 0
    ws = torch.empty((need,), device="cuda", dtype=torch.uint8)
    nbytes, counts = raw.count(grid, 0.0, ws)
    full = raw.emit(grid, 0.0, ws, nbytes, counts)
    rv, rf, rn = M.marching_cubes(grid.cpu().numpy(), 0.0, LO, HI)
    assert np.array_equal(full["f"], rf) and full["v"].shape == rv.shape
    for which in "vfn":
        one = raw.emit(grid, 0.0, ws, nbytes, counts, which)
        assert np.array_equal(one[which].view(np.uint32), full[which].view(np.uint32)), which


def test_two_rounds_through_one_workspace():
    """count + emit on one grid, then on a smaller, different one through the same workspace: what the first left behind does not show"""
    raw = _Raw()
    a = torch.as_tensor(M.checkerboard((24, 23, 22)), device="cuda")            # leaves almost every edge flagged
    b = torch.as_tensor(M.noise((5, 5, 41)), device="cuda")
    ws = torch.empty((raw.size(a.shape)[1],), device="cuda", dtype=torch.uint8)
    nbytes, counts = raw.count(a, 0.0, ws)
    first = raw.emit(a, 0.0, ws, nbytes, counts)
    assert np.array_equal(first["f"], M.marching_cubes(a.cpu().numpy(), 0.0, LO, HI)[1])
    nbytes, counts = raw.count(b, 0.0, ws)
    second = raw.emit(b, 0.0, ws, nbytes, counts)
    fresh = _gpu_mc(b.cpu().numpy(), 0.0)                                       # the same grid through a workspace of its own
    for k, want in zip("vfn", fresh):
        assert np.array_equal(second[k].view(np.uint32), want.view(np.uint32)), k
    assert np.array_equal(second["f"], M.marching_cubes(b.cpu().numpy(), 0.0, LO, HI)[1])


def test_empty_surface_emits_nothing():
    """V = F = 0 from the count phase; an emit call then launches nothing: the caller's arrays stay as they were"""
    raw = _Raw()
    for value in (1.0, -1.0):
        grid = torch.full((6, 7, 9), value, device="cuda")
        ws = torch.empty((raw.size(grid.shape)[1],), device="cuda", dtype=torch.uint8)
        nbytes, counts = raw.count(grid, 0.0, ws)
        assert (counts[0], counts[1]) == (0, 0)
        v = torch.full((1, 3), -7.0, device="cuda"); f = torch.full((1, 3), -7, device="cuda", dtype=torch.int32); n = v.clone()
        assert raw.call(grid, grid.shape, 0.0, ws, nbytes, counts, v, f, n) == 0
        assert (v == -7).all() and (f == -7).all() and (n == -7).all()


def test_size_and_workspace_refusals():
    raw = _Raw()
    # 1025 x 1024 x 256 > 2^28 points: refused before anything is allocated or launched (no grid, no workspace)
    assert raw.size((1025, 1024, 256)) == (raw.INVALID, 0)
    rc, need = raw.size((1024, 1024, 256))                                     # 2^28 exactly: the size query answers
    assert rc == 0 and need > 16 * 2 ** 28
    grid = torch.as_tensor(M.noise((8, 8, 16)), device="cuda")
    rc, need = raw.size(grid.shape)
    ws = torch.empty((need,), device="cuda", dtype=torch.uint8)
    nbytes, counts = C.c_size_t(need - 1), (C.c_int64 * 2)()
    assert raw.call(grid, grid.shape, 0.0, ws, nbytes, counts) == raw.INVALID   # one byte short
    nbytes = C.c_size_t(need)
    assert raw.call(grid, grid.shape, 0.0, ws, nbytes, counts) == 0 and counts[0] > 0


# ---- a non-finite sample stays local

@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_sample_stays_local(value):
    """One interior sample of the 17^3 noise grid set to NaN (never > tau: outside) or +inf (always inside).  Faces = the reference's on
    that grid.  Every vertex not on one of the sample's six edges, and every normal whose gradient stencil (the six neighbours of the
    edge's two ends) does not hold the sample, has the bits it has on the finite grid, vertex ids mapped by edge.  What the vertices
    and normals that do touch the sample hold is not asserted (include/knerf.h says so)."""
    base = M.noise((17, 17, 17))
    R = base.shape
    strides = np.array((R[1] * R[2], R[2], 1))
    inner = base[1:-1, 1:-1, 1:-1]
    i, j, k = (int(x[0]) + 1 for x in np.nonzero(inner > 0.0))                 # the first interior sample that is inside
    S = np.array((i, j, k))
    p0 = int(S @ strides)
    v1, f1, n1 = _gpu_mc(base, 0.0)
    (_, rf1, _), det1 = M.marching_cubes(base, 0.0, LO, HI, details=True)
    assert np.array_equal(f1, rf1)
    grid = base.copy()
    grid[i, j, k] = value
    v2, f2, n2 = _gpu_mc(grid, 0.0)
    (_, rf2, _), det2 = M.marching_cubes(grid, 0.0, LO, HI, details=True)
    assert np.array_equal(f2, rf2) and len(v2) == len(det2["edges"])
    e1, e2 = det1["edges"], det2["edges"]
    six = np.array([3 * p0 + a for a in range(3)] + [3 * (p0 - strides[a]) + a for a in range(3)])
    assert np.isin(np.setxor1d(e1, e2), six).all()                             # no other edge changes its state
    if np.isnan(value):
        assert np.setxor1d(e1, e2).size > 0                                    # the sample was inside: NaN moved it out
    common = np.setdiff1d(np.intersect1d(e1, e2), six)
    i1, i2 = np.searchsorted(e1, common), np.searchsorted(e2, common)
    assert np.array_equal(v1[i1].view(np.uint32), v2[i2].view(np.uint32))
    p, a = common // 3, common % 3
    P = np.stack(np.unravel_index(p, R), -1)
    Q = P + np.eye(3, dtype=np.int64)[a]
    touched = (np.abs(P - S).sum(1) <= 1) | (np.abs(Q - S).sum(1) <= 1)
    assert 0 < touched.sum() < 0.05 * len(common)
    assert np.array_equal(n1[i1][~touched].view(np.uint32), n2[i2][~touched].view(np.uint32))
