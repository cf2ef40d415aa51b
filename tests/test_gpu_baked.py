"""The baked field on the GPU (keras_nerf_amd/baked.py, csrc/baked.hip) against tests/baked_reference.py: the render kernel on a small
non-cubic lattice for every SH degree and kernel variant, exact empty-space skipping, termination, a closed form, the bake against the
network it was baked from, and persistence.

Measured on an MI355X (largest deviation from the fp64 marcher over the 150 rays; every degree and kernel variant within these):
image 4.7e-7 (bound 1e-5), depth 3.4e-6 (bound 2.1e-4 = 4 x the fp32 reference's own deviation; t reaches 21 on the non-unit rays),
opacity 5.4e-7 (bound 1e-5).  test_render_matches_the_fp64_marcher prints the figures of the run."""
import numpy as np
import pytest
import torch

from tests import baked_reference as R

pytestmark = pytest.mark.gpu

RES = (9, 7, 6)
LO, HI = (-1.0, -0.8, -0.6), (1.0, 0.8, 0.7)
STEP = 0.02
N_RAYS = 150
VARIANTS = {0: (0, 1), 1: (0, 1, 2), 2: (0, 1, 4), 3: (0, 1, 4)}      # lanes_per_ray values per degree (0: the default)


def _lattice(degree, seed=0, dense=1.0):
    rng = np.random.default_rng(100 + seed)
    sigma = rng.uniform(0.0, 30.0, RES).astype(np.float32) * np.float32(dense)
    sigma[0], sigma[-1], sigma[:, 0], sigma[:, -1], sigma[:, :, 0], sigma[:, :, -1] = 0, 0, 0, 0, 0, 0     # no jump at the box face
    sigma[3:6, 2:4, 2:4] = 0                                                                              # two empty interior cells
    K = (degree + 1) ** 2
    co = (rng.standard_normal(RES + (K, 3)) * 0.6).astype(np.float16)
    co[..., 0, :] += np.float16(1.5)
    return sigma, co


@pytest.fixture(scope="module")
def rays():
    rng = np.random.default_rng(7)
    lo, hi = np.array(LO), np.array(HI)
    mid = 0.5 * (lo + hi)
    o = np.zeros((N_RAYS, 3)); d = np.zeros((N_RAYS, 3))
    near = rng.uniform(0.0, 0.5, N_RAYS); far = rng.uniform(5.0, 6.5, N_RAYS)

    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)
    # 0..89 cross the box (the first ten through the empty block), from a sphere of radius 3
    o[:90] = mid + 3.0 * unit(rng.standard_normal((90, 3)))
    target = rng.uniform(lo + 0.1, hi - 0.1, (90, 3))
    block = lo + (np.array([4.0, 2.5, 2.5]) / (np.array(RES) - 1)) * (hi - lo)
    target[:10] = block + rng.uniform(-0.02, 0.02, (10, 3))
    d[:90] = unit(target - o[:90])
    # 90..109 miss it
    o[90:110] = mid + 3.0 * unit(rng.standard_normal((20, 3)))
    d[90:110] = unit(o[90:110] - mid + 0.3 * rng.standard_normal((20, 3)))
    # 110..129 start inside
    o[110:130] = rng.uniform(lo + 0.05, hi - 0.05, (20, 3)); d[110:130] = unit(rng.standard_normal((20, 3))); near[110:130] = 0.0
    # 130..137 one direction component exactly 0; 138..143 two (the last two start inside)
    for i in range(130, 138):
        a = i % 3
        o[i] = mid + 3.0 * unit(rng.standard_normal(3)); t = rng.uniform(lo + 0.2, hi - 0.2)
        o[i][a] = t[a]
        d[i] = t - o[i]; d[i][a] = 0.0; d[i] = unit(d[i])
    for i in range(138, 144):
        a = i % 3
        o[i] = rng.uniform(lo + 0.2, hi - 0.2); d[i] = 0.0; d[i][a] = 1.0 if i % 2 else -1.0
        if i < 142:
            o[i][a] = mid[a] - 3.0 * d[i][a]
        else:
            near[i] = 0.0
    # 144 parallel to the +y face just outside it, 145 in the plane of the +y face, 146..149 non-unit directions through the box
    o[144] = (-3.0, np.float32(HI[1]) + 1e-4, 0.1); d[144] = (1.0, 0.0, 0.0)
    o[145] = (-3.0, np.float32(HI[1]), 0.1); d[145] = (1.0, 0.0, 0.0)
    for i, s in zip(range(146, 150), (2.5, 0.3, 7.0, 1.0 / 3.0)):
        o[i] = mid + 3.0 * unit(rng.standard_normal(3))
        d[i] = unit(rng.uniform(lo + 0.2, hi - 0.2) - o[i]) * s
        near[i] /= s; far[i] /= s
    return {"o": o.astype(np.float32), "d": d.astype(np.float32), "near": near.astype(np.float32), "far": far.astype(np.float32)}


_refs = {}


def _reference(degree, rays, dense=1.0, termination=0.0):
    """the fp64 marcher and its own fp32 rounding error, computed once per case and shared"""
    key = (degree, dense, termination)
    if key not in _refs:
        sigma, co = _lattice(degree, dense=dense)
        cnt = []
        args = (sigma, co.astype(np.float64), LO, HI, rays["o"], rays["d"], rays["near"], rays["far"], STEP)
        r64 = R.march(*args, termination=termination, dtype=np.float64, count=cnt)
        r32 = R.march(*args, termination=termination, dtype=np.float32)
        scale = (1.0, float(rays["far"].max()), 1.0)
        bound = [max(1e-5 * s, 4.0 * float(np.abs(a.astype(np.float64) - b).max())) for a, b, s in zip(r32, r64, scale)]
        _refs[key] = (r64, bound, cnt)
    return _refs[key]


def _field(degree, dense=1.0):
    from keras_nerf_amd.baked import BakedField
    sigma, co = _lattice(degree, dense=dense)
    return BakedField.from_arrays(sigma, co, (LO, HI))


def _render(field, rays, **kw):
    out = field.render(rays["o"], rays["d"], rays["near"], rays["far"], step=STEP, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_render_matches_the_fp64_marcher(degree, rays):
    """every ray of the set, every output, every kernel variant of the degree; bound per output: max(1e-5 x scale, 4 x the fp32
    reference's own deviation from the fp64 reference)"""
    (img, dep, opa), bound, cnt = _reference(degree, rays)
    assert opa[:90].min() > 0.05 and opa[90:110].max() == 0 and opa[144] == 0          # the set does what it says
    field = _field(degree)
    sigma, co = _lattice(degree)
    assert torch.equal(field.sigma.cpu(), torch.as_tensor(sigma)) and field.sigma.dtype == torch.float32
    assert np.array_equal(field.coefficients.cpu().numpy().view(np.uint16), co.view(np.uint16))
    assert np.array_equal(field.occupied.cpu().numpy(), R.occupied_cells(sigma)) and not field.occupied.all()
    assert field.resolution == RES and field.sh_degree == degree and field.bounds == (LO, HI)
    for lanes in VARIANTS[degree]:
        out = _render(field, rays, lanes_per_ray=lanes, stats=True)
        assert out["image"].shape == (N_RAYS, 3) and out["depth"].shape == (N_RAYS,) and out["opacity"].shape == (N_RAYS,)
        errs = [float(np.abs(out[k].cpu().numpy().astype(np.float64) - ref).max()) for k, ref in
                (("image", img), ("depth", dep), ("opacity", opa))]
        print(f"degree {degree} lanes {lanes}: max |image, depth, opacity - fp64| = {errs}, bounds {bound}")
        for e, b, k in zip(errs, bound, ("image", "depth", "opacity")):
            assert e <= b, (degree, lanes, k, e, b)
        st = out["stats"].cpu().numpy()
        assert st[1] == cnt[1] and 0 < st[0] < st[1]


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_skipping_empty_cells_is_exact(degree, rays):
    field = _field(degree)
    for lanes in VARIANTS[degree]:
        for white in (False, True):
            a = _render(field, rays, lanes_per_ray=lanes, skip_empty=True, stats=True, white_background=white)
            b = _render(field, rays, lanes_per_ray=lanes, skip_empty=False, stats=True, white_background=white)
            for k in ("image", "depth", "opacity"):
                assert torch.equal(a[k], b[k]), (degree, lanes, k)
            sa, sb = a["stats"].cpu().numpy(), b["stats"].cpu().numpy()
            assert sa[0] < sb[0] <= sb[1] and sa[1] == sb[1], (sa, sb)


@pytest.mark.parametrize("degree", [1, 2])
def test_termination(degree, rays):
    (img, dep, opa), bound, _ = _reference(degree, rays)
    field = _field(degree)
    base = _render(field, rays, stats=True)
    zero = _render(field, rays, termination=0.0, stats=True)
    cut = _render(field, rays, termination=1e-3, stats=True)
    for k in ("image", "depth", "opacity", "stats"):
        assert torch.equal(base[k], zero[k]), k
    far = float(rays["far"].max())
    assert float((cut["image"] - base["image"]).abs().max()) <= 1e-3 + bound[0]
    assert float((cut["opacity"] - base["opacity"]).abs().max()) <= 1e-3 + bound[2]
    assert float((cut["depth"] - base["depth"]).abs().max()) <= 1e-3 * far
    assert int(cut["stats"][0]) <= int(base["stats"][0])
    # against the reference's own termination, and a dense field (sigma x 10) where rays do end early
    (img_t, dep_t, opa_t), bound_t, _ = _reference(degree, rays, dense=10.0, termination=1e-3)
    dense = _field(degree, dense=10.0)
    d0 = _render(dense, rays, stats=True)
    d1 = _render(dense, rays, termination=1e-3, stats=True)
    assert int(d1["stats"][0]) < int(d0["stats"][0])
    assert float((d1["image"] - d0["image"]).abs().max()) <= 1e-3 + bound_t[0]
    assert float((d1["opacity"] - d0["opacity"]).abs().max()) <= 1e-3 + bound_t[2]
    assert float((d1["depth"] - d0["depth"]).abs().max()) <= 1e-3 * far
    # a ray stops at the first sample with T < eps; one whose T passes eps within rounding may stop a sample apart from the
    # reference's, which moves the outputs by less than eps
    assert float(np.abs(d1["opacity"].cpu().numpy() - opa_t).max()) <= 1e-3 + bound_t[2]
    assert float(np.abs(d1["image"].cpu().numpy() - img_t).max()) <= 1e-3 + bound_t[0]


def test_constant_field_closed_form():
    """sigma0 on every lattice point and one colour: opacity = 1 - exp(-sigma0 L) to within sigma0 x step (the midpoint samples count
    the chord L to within one step), image = colour x opacity, white background: exactly 1 where the ray misses"""
    from keras_nerf_amd.baked import BakedField
    sigma0, step = 2.0, 0.01
    colour = np.array([0.25, 0.5, 0.75])
    co = np.zeros(RES + (9, 3), dtype=np.float16)
    co[..., 0, :] = (colour * 2.0 * np.sqrt(np.pi)).astype(np.float16)
    colour16 = co[0, 0, 0, 0].astype(np.float64) / (2.0 * np.sqrt(np.pi))
    field = BakedField.from_arrays(np.full(RES, sigma0, dtype=np.float32), co, (LO, HI))
    rng = np.random.default_rng(11)
    lo, hi = np.array(LO), np.array(HI)
    n = 70
    o = 0.5 * (lo + hi) + 3.0 * (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.standard_normal((n, 3)))
    tgt = rng.uniform(lo + 0.05, hi - 0.05, (n, 3))
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[60:] = -d[60:]                                                    # the last ten look away: they miss
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    o64, d64 = o32.astype(np.float64), d32.astype(np.float64)
    with np.errstate(divide="ignore"):
        t1, t2 = (lo - o64) / d64, (hi - o64) / d64
    tmin, tmax = np.minimum(t1, t2).max(axis=1), np.maximum(t1, t2).min(axis=1)
    L = np.maximum(0.0, tmax - np.maximum(tmin, 0.0)) * np.linalg.norm(d64, axis=1)
    assert (L[:60] > 0.1).all() and (L[60:] == 0).all()
    want = 1.0 - np.exp(-sigma0 * L)
    for white in (False, True):
        out = field.render(o32, d32, 0.0, 6.0, step=step, white_background=white)
        opa = out["opacity"].cpu().numpy().astype(np.float64)
        img = out["image"].cpu().numpy().astype(np.float64)
        assert np.abs(opa - want).max() <= sigma0 * step
        bg = (1.0 - opa)[:, None] if white else 0.0
        assert np.abs(img - (colour16[None, :] * want[:, None] + bg)).max() <= sigma0 * step
        if white:
            assert (img[60:] == 1.0).all() and (opa[60:] == 0.0).all()
        else:
            assert (img[60:] == 0.0).all()


def test_bake_against_the_network():
    """tolerance per coefficient: 2^-10 |value| (fp16 rounding) + 2^-24 D max|P| (the fp32 sum).  A plain fp32 fma chain over the 32
    directions missed it by 4.2e-8 on one coefficient near zero (error 8e-7: the partial sums reach 1 ... 2 before they cancel); the
    bake sums with compensation (knerf_baked_project with its second buffer) and passes."""
    from keras_nerf_amd.baked import fit_directions
    from keras_nerf_amd.runtime import occupancy_from_grid
    from tests.test_gpu_query import _nerf
    nerf, _ = _nerf()
    res, bounds = (12, 10, 9), ((-1.5,) * 3, (1.5,) * 3)
    grid = nerf.density_grid(res, bounds)
    tau = float(np.quantile(grid.cpu().numpy(), 0.6))
    field = nerf.bake(resolution=res, bounds=bounds, sh_degree=2, n_directions=32, sigma_threshold=tau)
    want_sigma = torch.where(grid > tau, grid, torch.zeros_like(grid))
    assert torch.equal(field.sigma, want_sigma)
    occ = occupancy_from_grid(want_sigma, 0.0, 0)
    assert np.array_equal(field.occupied.cpu().numpy(), occ) and np.array_equal(occ, R.occupied_cells(want_sigma.cpu().numpy()))
    assert occ.any() and not occ.all()
    touched = R.touched_points(occ)
    assert touched.any() and not touched.all()
    pts = R.lattice_points(res, *bounds)[touched]
    # these are the points at which knerf_query_grid evaluated sigma: the point query gives the grid's bits
    assert torch.equal(nerf.query(pts, None)[1].reshape(-1), grid[torch.as_tensor(touched, device=grid.device)])
    dirs, P = fit_directions(2, 32)
    dref, Pref = R.fit_matrix(2, 32)
    assert np.abs(dirs - dref).max() < 1e-12 and np.abs(P - Pref).max() < 1e-10
    P32 = P.astype(np.float32).astype(np.float64)                       # the matrix as the device holds it
    rgb = np.stack([nerf.query(pts, dirs[j].astype(np.float32))[0].cpu().numpy().astype(np.float64) for j in range(32)])   # [D,n,3]
    want = np.einsum("kj,jnc->nkc", P32, rgb)
    got = field.coefficients.cpu().numpy().astype(np.float64)
    tol = 2.0 ** -10 * np.abs(want) + 2.0 ** -24 * 32 * np.abs(P32).max()
    assert (np.abs(got[touched] - want) <= tol).all(), float((np.abs(got[touched] - want) - tol).max())
    assert not field.coefficients.cpu().numpy().view(np.uint16)[~touched].any()              # exactly +0 everywhere else
    # the work list in eleven slabs (accumulators reused and packed per slab) gives the same records
    from keras_nerf_amd.baked import bake
    slabs = bake(nerf, resolution=res, bounds=bounds, sh_degree=2, n_directions=32, sigma_threshold=tau, slab_bytes=24 * 9 * 100)
    assert int(touched.sum()) > 1000 and torch.equal(slabs._records, field._records) and torch.equal(slabs._words, field._words)
    # degree 0: the DC coefficient times Y_0 is the colour along the zero direction
    f0 = nerf.bake(resolution=res, bounds=bounds, sh_degree=0, sigma_threshold=tau)
    assert torch.equal(f0.sigma, want_sigma)
    rgb0 = nerf.query(pts, None)[0].cpu().numpy().astype(np.float64)
    got0 = f0.coefficients.cpu().numpy().astype(np.float64)
    assert got0.shape == res + (1, 3) and not got0[~touched].any()
    y0 = 1.0 / (2.0 * np.sqrt(np.pi))
    assert (np.abs(got0[touched][:, 0, :] * y0 - rgb0) <= 2.0 ** -10 * rgb0 + 2.0 ** -22).all()
    # and the baked field renders
    o = np.array([[0.0, 0.0, 4.0]] * 5, dtype=np.float32); d = np.array([[0.0, 0.0, -1.0]] * 5, dtype=np.float32)
    o[:, 0] = np.linspace(-1.0, 1.0, 5)
    a = field.render(o, d, 2.0, 6.0, stats=True)
    b = field.render(o, d, 2.0, 6.0, skip_empty=False, stats=True)
    assert all(torch.equal(a[k], b[k]) for k in ("image", "depth", "opacity")) and torch.isfinite(a["image"]).all()
    assert int(a["stats"][0]) <= int(b["stats"][0]) and float(a["opacity"].max()) > 0


def test_save_load_and_repeat(tmp_path, rays):
    from keras_nerf_amd.baked import BakedField
    field = _field(2)
    a = _render(field, rays, white_background=True, outputs=("image", "opacity"))
    b = _render(field, rays, white_background=True, outputs=("image", "opacity"))
    assert sorted(a) == ["image", "opacity"] and all(torch.equal(a[k], b[k]) for k in a)
    path = str(tmp_path / "field.npz")
    field.save(path)
    again = BakedField.load(path)
    assert again.resolution == field.resolution and again.bounds == field.bounds and again.sh_degree == 2
    assert torch.equal(again.sigma, field.sigma) and torch.equal(again.coefficients, field.coefficients)
    assert torch.equal(again.occupied, field.occupied)
    c = _render(again, rays, white_background=True, outputs=("image", "opacity"))
    assert all(torch.equal(a[k], c[k]) for k in a)
    # scalar near / far and the default step (half the smallest cell edge)
    e = field.render(rays["o"], rays["d"], 0.0, 6.0)
    f = field.render(rays["o"], rays["d"], np.zeros(N_RAYS, np.float32), np.full(N_RAYS, 6.0, np.float32), step=0.5 * float(min(field.cell_size)))
    assert all(torch.equal(e[k], f[k]) for k in e)
    with pytest.raises(ValueError):
        field.render(rays["o"], rays["d"], 0.0, 6.0, step=-1.0)
    with pytest.raises(ValueError):
        field.render(rays["o"], rays["d"], 0.0, 6.0, outputs=("rgb",))


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_padding_of_a_loaded_file_is_never_read_as_data(degree, tmp_path, rays):
    """a file whose record padding holds NaN halfs renders, with every kernel variant, the bits of the clean field; a path without
    the .npz suffix is written and read as given"""
    from keras_nerf_amd.baked import BakedField
    field = _field(degree)
    path = str(tmp_path / "scene")
    field.save(path)
    assert BakedField.load(path).resolution == RES
    with np.load(path) as z:
        data = {k: z[k] for k in z.files}
    K = (degree + 1) ** 2
    pad = data["records"][:, 4 + 6 * K:]
    assert pad.shape[1] >= 4 and not pad.any()
    pad[:, 0::2], pad[:, 1::2] = 0x00, 0x7e                      # fp16 NaN in every padding slot
    dirty_path = str(tmp_path / "dirty.npz")
    np.savez(dirty_path, **data)
    dirty = BakedField.load(dirty_path)
    for lanes in VARIANTS[degree]:
        a, b = _render(field, rays, lanes_per_ray=lanes), _render(dirty, rays, lanes_per_ray=lanes)
        for k in ("image", "depth", "opacity"):
            assert torch.isfinite(b[k]).all() and torch.equal(a[k], b[k]), (degree, lanes, k)
