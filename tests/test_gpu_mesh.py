"""knerf_marching_cubes (csrc/mesh.hip) against the NumPy reference (tests/mc_reference.py), and NeRF.extract_mesh on the GPU."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import mc_reference as M

pytestmark = pytest.mark.gpu
LO, HI = (-1.5,) * 3, (1.5,) * 3
EXT = 3.0


def _gpu_mc(grid, tau, lo=LO, hi=HI):
    from keras_nerf_amd.runtime import marching_cubes
    v, f, n = marching_cubes(torch.as_tensor(grid, device="cuda"), tau, lo, hi)
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()


def _same_as_reference(grid, tau, lo=LO, hi=HI, ref=None):
    """ref: M.marching_cubes(grid, tau, lo, hi) where the caller has it already"""
    v, f, n = _gpu_mc(grid, tau, lo, hi)
    rv, rf, rn = ref if ref is not None else M.marching_cubes(grid, tau, lo, hi)
    assert np.array_equal(f, rf), (f.shape, rf.shape)
    assert v.shape == rv.shape and np.abs(v - rv).max(initial=0) <= 1e-6 * EXT
    assert np.abs(n - rn).max(initial=0) <= 1e-6 * EXT
    return v, f, n


def test_sphere_matches_the_reference_and_is_closed():
    v, f, n = _same_as_reference(M.sphere(128, 1.0), 0.0)
    M.check_closed_manifold(f, len(v))
    assert M.euler(f, len(v)) == 2
    assert (np.einsum("ij,ij->i", n, v / np.linalg.norm(v, axis=1, keepdims=True)) > 0.99).all()
    v2, f2, n2 = _gpu_mc(M.sphere(128, 1.0), 0.0)                           # a second call: identical arrays
    assert np.array_equal(v, v2) and np.array_equal(f, f2) and np.array_equal(n, n2)


def test_odd_grid_and_bounds_match_the_reference():
    s = M.torus(61)[:, :50, 3:]
    _same_as_reference(np.ascontiguousarray(s), 0.05, (-1.0, -0.5, -2.0), (1.0, 0.7, 1.0))


def test_network_density_grid_matches_the_reference():
    from tests.test_gpu_query import _nerf
    nerf, _ = _nerf()
    g = nerf.density_grid(64)
    gn = g.cpu().numpy()
    tau = float(np.quantile(gn, 0.7))
    assert tau < gn.max()
    v, f, n = _same_as_reference(gn, tau)
    assert len(f) > 100
    # NeRF.extract_mesh gives the same mesh; vertex colours are query(vertices, -normals) bit for bit
    ev, ef, en, ec = nerf.extract_mesh(tau, 64, vertex_colors=True)
    assert np.array_equal(ef.cpu().numpy(), f) and np.array_equal(ev.cpu().numpy(), v) and np.array_equal(en.cpu().numpy(), n)
    rgb, _ = nerf.query(ev, -en)
    assert torch.equal(ec, rgb)
    # above the maximum: an empty surface, not an error
    ev, ef, en = nerf.extract_mesh(float(gn.max()) + 1.0, 64)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and en.shape == (0, 3)


def test_marching_cubes_argument_errors():
    from keras_nerf_amd.runtime import marching_cubes
    g = torch.zeros((4, 4, 4), device="cuda")
    for bad in (g.double(), g.transpose(0, 2), torch.zeros((1, 4, 4), device="cuda"), torch.zeros((4, 4), device="cuda")):
        with pytest.raises(ValueError):
            marching_cubes(bad, 0.0, LO, HI)
    with pytest.raises(ValueError):
        marching_cubes(g, 0.0, (0, 0, 0), (1, 1, 0))


def test_save_ply_of_an_extracted_mesh(tmp_path):
    from keras_nerf_amd.io.ply import save_ply
    from tests.test_mesh_table import _read_ply
    v, f, n = _gpu_mc(M.sphere(32, 1.0), 0.0)
    save_ply(str(tmp_path / "s.ply"), v, f, n)
    r = _read_ply(str(tmp_path / "s.ply"))
    assert len(r["vertex"]) == len(v) and np.array_equal(r["face"]["i"], f)
