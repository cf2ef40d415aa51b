"""The host side of the baked field (keras_nerf_amd/baked.py) against tests/baked_reference.py: the SH basis, the fit matrix, the record
layout and the argument checks.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from keras_nerf_amd import baked as B
from tests import baked_reference as R


def test_sh_basis_is_orthonormal_under_an_exact_quadrature():
    """Gauss-Legendre in cos(theta) (24 nodes: exact to degree 47) times a uniform rule in phi (16 nodes: exact for |m| <= 15): products
    of two degree-3 harmonics have degree 6 and |m| <= 6"""
    x, w = np.polynomial.legendre.leggauss(24)
    phi = 2 * np.pi * np.arange(16) / 16
    ct, ph = np.meshgrid(x, phi, indexing="ij")
    st = np.sqrt(1 - ct * ct)
    v = np.stack([st * np.cos(ph), st * np.sin(ph), ct], axis=-1)
    wt = np.broadcast_to(w[:, None] * (2 * np.pi / 16), ct.shape)
    for basis in (R.real_sh, B.sh_basis):
        Y = basis(v, 3)
        G = np.einsum("ijk,ijl,ij->kl", Y, Y, wt)
        assert np.abs(G - np.eye(16)).max() < 1e-12
    # the package's basis is the reference's, and lower degrees are its leading blocks
    assert np.abs(B.sh_basis(v, 3) - R.real_sh(v, 3)).max() < 1e-15
    for deg in range(4):
        assert np.array_equal(B.sh_basis(v, deg), B.sh_basis(v, 3)[..., :(deg + 1) ** 2])


def test_kernel_constants_agree_with_the_reference():
    """the literals of sh_eval (csrc/baked_common.h: the one definition every baked*.hip uses), read from the source, against the closed
    forms"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "baked_common.h")).read()
    body = src[src.index("void sh_eval"):src.index("template <int CTRL>")]
    got = [float(m) for m in re.findall(r"Y\[\d+\] = ([0-9.]+)f", body)]
    pi = np.pi
    want = [0.5 / np.sqrt(pi)] + [np.sqrt(3 / (4 * pi))] * 3 + \
        [0.5 * np.sqrt(15 / pi)] * 2 + [0.25 * np.sqrt(5 / pi), 0.5 * np.sqrt(15 / pi), 0.25 * np.sqrt(15 / pi)] + \
        [0.25 * np.sqrt(35 / (2 * pi)), 0.5 * np.sqrt(105 / pi), 0.25 * np.sqrt(21 / (2 * pi)), 0.25 * np.sqrt(7 / pi),
         0.25 * np.sqrt(21 / (2 * pi)), 0.25 * np.sqrt(105 / pi), 0.25 * np.sqrt(35 / (2 * pi))]
    assert len(got) == 16
    assert np.allclose(got, want, rtol=1e-15, atol=0)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_fit_matrix_inverts_the_basis(degree):
    dirs, P = B.fit_directions(degree)
    dref, Pref = R.fit_matrix(degree)
    K = (degree + 1) ** 2
    assert dirs.shape == (R.default_n_directions(degree), 3) and P.shape == (K, dirs.shape[0])
    assert np.abs(dirs - dref).max() < 1e-12 and np.abs(P - Pref).max() < 1e-10
    if degree == 0:
        assert np.array_equal(dirs, np.zeros((1, 3)))
        Y = R.real_sh(np.array([[0.0, 0.0, 1.0]]), 0)
    else:
        assert np.abs(np.linalg.norm(dirs, axis=1) - 1).max() < 1e-12
        Y = R.real_sh(dirs, degree)
    assert np.abs(P @ Y - np.eye(K)).max() < 1e-10
    # a function in the span comes back with its coefficients
    c = np.random.default_rng(degree).standard_normal((K, 3))
    assert np.abs(P @ (Y @ c) - c).max() < 1e-10


def test_records_round_trip_bit_for_bit():
    rng = np.random.default_rng(3)
    for degree, size in ((0, 16), (1, 32), (2, 64), (3, 112)):
        K = (degree + 1) ** 2
        assert B.record_bytes(degree) == size
        sigma = rng.uniform(0, 30, (5, 4, 3)).astype(np.float32)
        co = rng.standard_normal((5, 4, 3, K, 3)).astype(np.float16)
        co.reshape(-1)[:4] = np.array([0.0, -0.0, 65504.0, 6e-8], dtype=np.float16)
        rec = B.pack_records(sigma, co)
        assert rec.shape == (60, size) and rec.dtype == np.uint8
        s2, c2 = B.unpack_records(rec, degree)
        assert np.array_equal(s2.view(np.uint32), sigma.reshape(-1).view(np.uint32))
        assert np.array_equal(c2.view(np.uint16), co.reshape(-1, K, 3).view(np.uint16))
        assert not rec[:, 4 + 6 * K:].any()                         # padding
        # [k][c] order behind the four bytes of sigma
        assert np.array_equal(rec[7, 4:10].view(np.float16), co.reshape(-1, K, 3)[7, 0])


def test_bad_arguments_are_value_errors():
    ok_bounds = ((-1.0,) * 3, (1.0,) * 3)
    for deg in (-1, 4, 1.5, True, None):
        with pytest.raises(ValueError, match="sh_degree"):
            B.check_degree(deg)
        with pytest.raises(ValueError, match="sh_degree"):
            B.fit_directions(deg)
    for deg, D in ((1, 7), (2, 17), (3, 31), (2, 0), (2, 20.0)):
        with pytest.raises(ValueError, match="n_directions"):
            B.fit_directions(deg, D)
    assert B.fit_directions(2, 18)[1].shape == (9, 18)
    for res in (1, 1026, (8, 1, 8), (8, 8), (8, 8, 2000), 8.5, "8"):
        with pytest.raises(ValueError, match="resolution"):
            B.check_lattice_spec(res, ok_bounds, 2)
    assert B.check_lattice_spec(1025, ok_bounds, 3)[0] == (1025,) * 3
    assert B.check_lattice_spec((2, 3, 4), ok_bounds, 0)[0] == (2, 3, 4)
    for bounds in (((0, 0, 0), (1, 1, 0)), ((0, 0, 0), (1, -1, 1)), ((0, 0), (1, 1)), ((0, 0, 0), (1, 1, np.inf)), None):
        with pytest.raises(ValueError, match="bounds"):
            B.check_lattice_spec(8, bounds, 2)
    # the 2^40-byte bound of the record table (no lattice of 1025^3 points reaches it; the table size is checked on its own)
    assert B.check_table_size((1 << 40) // 64 - 1, 2) == (1 << 40) - 64
    for n, deg in (((1 << 40) // 64, 2), ((1 << 40) // 16, 0), ((1 << 40) // 112 + 1, 3)):
        with pytest.raises(ValueError, match="2\\^40"):
            B.check_table_size(n, deg)
    for step in (0, -0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match="step"):
            B.check_render_args(step, 0.0, ("image",), 2)
    for term in (-1e-3, 1.0, 2, np.nan):
        with pytest.raises(ValueError, match="termination"):
            B.check_render_args(None, term, ("image",), 2)
    for outs in (("image", "weights"), (), "rgb", ("depth", "depth")):
        with pytest.raises(ValueError, match="outputs"):
            B.check_render_args(None, 0.0, outs, 2)
    with pytest.raises(ValueError, match="lanes_per_ray"):
        B.check_render_args(None, 0.0, ("image",), 2, lanes_per_ray=2)
    assert B.check_render_args(0.01, 0.5, "depth", 1, 2) == ("depth",)


def test_nerf_bake_checks_its_arguments_before_it_needs_a_device():
    from keras_nerf_amd.model.nerf.nerf import NeRF
    n = NeRF()
    with pytest.raises(ValueError, match="sh_degree"):
        n.bake(sh_degree=4)
    with pytest.raises(ValueError, match="resolution"):
        n.bake(resolution=1026)
    with pytest.raises(ValueError, match="n_directions"):
        n.bake(sh_degree=2, n_directions=17)
    with pytest.raises(ValueError, match="bounds"):
        n.bake(bounds=((0, 0, 0), (1, 1, 0)))
    for thr in (-1e-3, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="sigma_threshold"):
            n.bake(resolution=8, sigma_threshold=thr)
    with pytest.raises(RuntimeError, match="not compiled"):
        n.bake(resolution=8)


def test_a_negative_threshold_is_refused_before_any_device_work():
    """negative densities would be stored under it: a cell with only negative corners has no occupancy bit but a non-zero trilinear
    sigma, and skipping would no longer be exact"""
    sigma = np.ones((3, 3, 3), dtype=np.float32)
    co = np.zeros((3, 3, 3, 4, 3), dtype=np.float16)
    for thr in (-1.0, -1e-30, float("nan")):
        with pytest.raises(ValueError, match="sigma_threshold"):
            B.BakedField.from_arrays(sigma, co, ((0, 0, 0), (1, 1, 1)), sigma_threshold=thr)
    assert B.check_threshold(0) == 0.0 and B.check_threshold(np.float32(2.5)) == 2.5


def test_load_refuses_a_file_that_is_not_a_baked_field(tmp_path):
    path = str(tmp_path / "other.npz")
    np.savez(path, records=np.zeros((8, 64), np.uint8))
    with pytest.raises(ValueError, match="not a baked field"):
        B.BakedField.load(path)


def test_the_library_refuses_bad_arguments_before_any_launch():
    """KNERF_ERR_INVALID from the three entry points with no device behind the pointers (nothing is dereferenced on the host)"""
    from keras_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)                                     # never dereferenced: every call below is refused first
    INV = _lib.KNERF_ERR_INVALID
    assert lib.knerf_baked_project(None, p, p, 5, 20, 0, 10, p, None) == INV           # K not a square of 1..4
    assert lib.knerf_baked_project(None, p, p, 9, 20, 20, 10, p, p) == INV          # j outside [0, D)
    assert lib.knerf_baked_project(None, None, p, 9, 20, 0, 10, p, None) == INV
    assert lib.knerf_baked_project(None, p, p, 9, 20, 0, (1 << 40) // 108 + 1, p, None) == INV
    assert lib.knerf_baked_pack(None, p, p, None, None, (1 << 40) // 64, (1 << 40) // 64, 2, p) == INV      # the 2^40 bound
    assert lib.knerf_baked_pack(None, p, p, None, None, 10, 10, 4, p) == INV
    assert lib.knerf_baked_pack(None, p, p, None, None, 5, 10, 2, p) == INV            # no index: n must be n_points
    assert lib.knerf_baked_pack(None, p, p, None, p, 11, 10, 2, p) == INV

    def field(res=(9, 7, 6), deg=2, lo=(-1, -1, -1), hi=(1, 1, 1), bits=256):
        return _lib.KnerfBakedField(C.c_void_p(256), C.c_void_p(bits) if bits else None, (C.c_int32 * 3)(*res), deg,
                                    (C.c_float * 3)(*lo), (C.c_float * 3)(*hi))

    def render(f, step=0.01, term=0.0, flags=2, n=10, image=p):
        return lib.knerf_baked_render(None, C.byref(f), p, p, None, None, 0.0, 1.0, n, step, term, flags, image, None, None, None)
    assert render(field(deg=4)) == INV and render(field(deg=-1)) == INV
    assert render(field(res=(9, 1, 6))) == INV and render(field(res=(1026, 7, 6))) == INV
    assert render(field(hi=(1, -1, 1))) == INV and render(field(hi=(1, float("nan"), 1))) == INV
    assert render(field(), step=0.0) == INV and render(field(), step=-1.0) == INV and render(field(), step=float("inf")) == INV
    assert render(field(), term=1.0) == INV and render(field(), term=-0.5) == INV
    assert render(field(), flags=4) == INV                                       # unknown flag bit
    assert render(field(), flags=2 | (2 << 8)) == INV                            # degree 2 has no 2-lane kernel
    assert render(field(bits=0), flags=2) == INV                                 # skipping needs the bits
    assert render(field(), image=None) == INV                                    # nothing to write
    assert render(field(), n=0) == 0                                             # no rays: nothing to do
