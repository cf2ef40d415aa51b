"""Camera models on the GPU: the kernels of csrc/rays_cam.hip against the fp64 restatements of tests/camera_reference.py and, where
they overlap, against the plain and the ray-model kernels bit for bit; then a transforms.json scene with distortion keys through the
loader and `fit`.

Shapes: V = 3 views of 12 x 20 pixels, N = 8 samples, the poses of tests/test_gpu_forward_facing.py; the camera sets of
camera_reference.SETS, each with pixel_offset 0 and 0.5.  tests/test_cameras_host.py shows that every set is invertible over the whole
grid, so no pixel is excluded anywhere, and that the float32 mirror of the kernels' arithmetic stays within a fifth of each bound
used here.  Depth is compared relative to the point's distance from the camera (see that file's docstring); for the cameras that
look along -z only it is also compared relative to itself."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import camera_reference as CR
from tests import forward_facing_reference as FF

pytestmark = pytest.mark.gpu
V, H, W, N = CR.V, CR.H, CR.W, CR.N
P = V * H * W
FOCAL = 18.0
CASES = [(name, off) for name in CR.SETS for off in CR.OFFSETS]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(x, y) and (x.dtype != torch.float32 or torch.equal(_bits(x), _bits(y))) for x, y in zip(a, b)) and len(a) == len(b)


def _ray_model(ndc=0, spacing=0, ndc_near=1.0):
    from keras_nerf_amd import _lib
    return _lib.KnerfRayModel(ndc, spacing, ndc_near)


def _camera(name, offset=0.0, model=None):
    from keras_nerf_amd.data.cameras import CameraModel
    m, fx, fy, cx, cy, c = CR.SETS[name]
    return CameraModel(model or m, fx, fy, cx, cy, c, pixel_offset=offset)


def _per_view(offset=0.5):
    """intrinsics, mild and strong as the cameras of views 0, 1, 2 (the pinhole set restated as opencv with zero coefficients)"""
    from keras_nerf_amd.data.cameras import CameraModel
    rows = [CR.SETS[k] for k in ("intrinsics", "mild", "strong")]
    return CameraModel("opencv", [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows],
                       [list(r[5]) + [0.0] * (5 - len(r[5])) for r in rows], pixel_offset=offset)


def _err(got, want):
    return float(np.abs(got.double().cpu().numpy() - want).max())


@pytest.fixture(scope="module")
def ctx():
    from keras_nerf_amd.runtime import KnerfContext
    c = KnerfContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene(ctx):
    """cameras, images, injected noise and the plain kernels' sample positions, shared and left unchanged"""
    g = torch.Generator(device="cuda").manual_seed(5)
    poses = FF.random_poses(V, FF.GPU_POSE_SEED)
    c2w = torch.as_tensor(poses, device="cuda")
    noise = torch.rand((V, H, W, N), device="cuda", generator=g)
    images = torch.rand((V, H, W, 4), device="cuda", generator=g)
    t = ctx.generate_rays(c2w, FOCAL, H, W, 2.0, 6.0, N, noise)[2]
    return dict(poses=poses, c2w=c2w, noise=noise, images=images, t=t, noise64=noise.double().cpu().numpy())


def test_the_plain_camera_writes_the_bits_of_the_plain_and_the_ray_model_kernels(ctx, scene):
    from keras_nerf_amd.data.cameras import CameraModel
    cam = CameraModel.from_focal(FOCAL, W, H)
    c2w, images = scene["c2w"], scene["images"]
    ranges = {None: (2.0, 6.0), "linear": (2.0, 6.0), "disparity": (2.0, 6.0), "ndc": (0.0, 1.0)}
    models = {None: None, "linear": _ray_model(), "disparity": _ray_model(spacing=1), "ndc": _ray_model(ndc=1)}
    for kw in (dict(noise=scene["noise"]), dict(noise=None, seed=77, stream_id=3), dict(noise=None, seed=2 ** 40 + 1, stream_id=2 ** 33)):
        for key, m in models.items():
            near, far = ranges[key]
            want = ctx.generate_rays(c2w, FOCAL, H, W, near, far, N, **kw) if m is None else ctx.generate_rays_ext(c2w, FOCAL, H, W, near, far, N, m, **kw)
            got = ctx.generate_rays_cam(c2w, cam, H, W, near, far, N, m, **kw)
            assert _same(want, got), (key, kw.get("seed"))
    n, first = 704, 9
    for kw in (dict(noise=torch.rand((n, N), device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))),
               dict(noise_stream=0), dict(noise_stream=2 ** 33 + 5)):
        for seed, epoch in ((0, 0), (2 ** 40 + 9, 4)):
            for key, m in models.items():
                near, far = ranges[key]
                extra = {} if m is None else {"ray_model": m}
                want = ctx.draw_ray_batch(images, c2w, FOCAL, near, far, N, seed, epoch, first, n, want_index=True, **extra, **kw)
                got = ctx.draw_ray_batch(images, c2w, None, near, far, N, seed, epoch, first, n, want_index=True, camera=cam, **extra, **kw)
                assert _same(want, got), (key, seed, epoch)
    # three channels, no index
    rgb = images[..., :3].contiguous()
    want = ctx.draw_ray_batch(rgb, c2w, FOCAL, 2.0, 6.0, N, 1, 0, 0, 64, noise_stream=1)
    got = ctx.draw_ray_batch(rgb, c2w, None, 2.0, 6.0, N, 1, 0, 0, 64, noise_stream=1, camera=cam)
    assert len(got) == 4 and _same(want, got)


@pytest.mark.parametrize("name,offset", CASES)
def test_every_camera_set_matches_the_fp64_reference(ctx, scene, name, offset):
    """max |d - d64| <= 2e-6 and | |d| - 1 | <= 1e-6 on unit vectors: 14x what the float32 mirror of the same arithmetic does (1.4e-7
    on the distorted pinhole sets); a wrong sign, a swapped coefficient, a missing offset or two Newton steps instead of eight are off
    by orders of magnitude"""
    cam = _camera(name, offset)
    o, d, t = ctx.generate_rays_cam(scene["c2w"], cam, H, W, 2.0, 6.0, N, None, scene["noise"])
    o64, d64 = CR.camera_rays(CR.SETS[name], offset, scene["poses"])
    assert torch.equal(_bits(o), _bits(scene["c2w"][:, None, None, :3, 3].expand(V, H, W, 3)))          # the translation's bits
    err, unit = _err(d, d64), float((d.double().norm(dim=-1) - 1).abs().max())
    print(f"{name} offset {offset}: max |d - d64| = {err:.3g}, max ||d| - 1| = {unit:.3g}")
    assert err <= CR.BOUND_DIRECTION, err
    assert unit <= CR.BOUND_UNIT, unit
    assert torch.equal(_bits(t), _bits(scene["t"]))                                                       # sample positions: the plain kernel's
    # disparity spacing works with every camera: the rays stay, the positions are those of the ray-model kernel
    m = _ray_model(spacing=1)
    od, dd, td = ctx.generate_rays_cam(scene["c2w"], cam, H, W, 2.0, 6.0, N, m, scene["noise"])
    assert torch.equal(_bits(od), _bits(o)) and torch.equal(_bits(dd), _bits(d))
    assert torch.equal(_bits(td), _bits(ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 2.0, 6.0, N, m, scene["noise"])[2]))


def test_a_per_view_table_equals_three_shared_camera_calls(ctx, scene):
    from keras_nerf_amd.data.cameras import CameraModel
    from keras_nerf_amd.data.rays import RaysGenerator
    per = _per_view()
    c2w, noise = scene["c2w"], scene["noise"]
    o, d, t = ctx.generate_rays_cam(c2w, per, H, W, 2.0, 6.0, N, None, noise)
    for v, name in enumerate(("intrinsics", "mild", "strong")):
        so, sd, st = ctx.generate_rays_cam(c2w[v:v + 1], _camera(name, 0.5, model="opencv"), H, W, 2.0, 6.0, N, None, noise[v:v + 1])
        assert torch.equal(_bits(so[0]), _bits(o[v])) and torch.equal(_bits(sd[0]), _bits(d[v])) and torch.equal(_bits(st[0]), _bits(t[v])), name
        assert torch.equal(_bits(per.select([v]).device_table()), _bits(_camera(name, 0.5, model="opencv").device_table()))
    # zero coefficients leave Newton's iterate where it starts: the promoted pinhole row writes the pinhole kernel's bits
    assert torch.equal(_bits(ctx.generate_rays_cam(c2w[:1], _camera("intrinsics", 0.5), H, W, 2.0, 6.0, N, None, noise[:1])[1][0]), _bits(d[0]))
    assert not torch.equal(d[1], ctx.generate_rays_cam(c2w[1:2], _camera("strong", 0.5), H, W, 2.0, 6.0, N, None, noise[1:2])[1][0])
    # the public class: rows gathered by view_index
    rg = RaysGenerator(None, W, H, 2.0, 6.0, N, camera=per)
    sel = [2, 0]
    go, gd, gt = rg(c2w[sel], noise=noise[sel], view_index=sel)
    assert torch.equal(_bits(go), _bits(o[sel])) and torch.equal(_bits(gd), _bits(d[sel])) and torch.equal(_bits(gt), _bits(t[sel]))
    go, gd, _ = rg(c2w[sel], noise=noise[sel], view_index=torch.as_tensor(sel, device="cuda"))
    assert torch.equal(_bits(go), _bits(o[sel])) and torch.equal(_bits(gd), _bits(d[sel]))
    assert torch.equal(_bits(rg(c2w, noise=noise)[1]), _bits(d))                                           # B = the table's rows: row v for view v
    g1 = rg(c2w[2], noise=noise[2], view_index=[2])
    assert g1[0].shape == (H, W, 3) and torch.equal(_bits(g1[1]), _bits(d[2]))
    with pytest.raises(ValueError):
        rg(c2w[sel], noise=noise[sel])                                                                     # two matrices, three rows, no view_index
    with pytest.raises(ValueError):
        rg(c2w[sel], noise=noise[sel], view_index=[0, 3])
    with pytest.raises(ValueError):
        RaysGenerator(None, W, H, 0.0, 1.0, N, ndc=True, camera=per)
    with pytest.raises(ValueError):
        RaysGenerator(None, W, H, 0.0, 1.0, N, ndc=True, camera=_camera("fisheye"))
    with pytest.raises(ValueError, match="fold|invertible"):
        RaysGenerator(None, W, H, 2.0, 6.0, N, camera=CameraModel("opencv", 11.0, 10.5, 9.4, 6.3, (-0.6,)))


@pytest.mark.parametrize("table", ["shared", "per_view"])
def test_a_ray_batch_holds_the_view_rays_bit_for_bit(ctx, scene, table):
    cam = _camera("strong", 0.5) if table == "shared" else _per_view()
    c2w, images = scene["c2w"], scene["images"]
    vo, vd, _ = ctx.generate_rays_cam(c2w, cam, H, W, 2.0, 6.0, N, None, scene["noise"])
    g = torch.Generator(device="cuda").manual_seed(6)
    for seed, epoch, first, n in ((0, 0, 0, P), (5, 3, 17, 700), (2 ** 40 + 9, 2 ** 33 + 1, P - 300, 300)):
        noise = torch.rand((n, N), device="cuda", generator=g)
        o, d, t, target, index = ctx.draw_ray_batch(images, c2w, None, 2.0, 6.0, N, seed, epoch, first, n, noise=noise, want_index=True, camera=cam)
        assert len(torch.unique(index)) == n and int(index.min()) >= 0 and int(index.max()) < P
        assert torch.equal(_bits(o), _bits(vo.reshape(P, 3)[index])) and torch.equal(_bits(d), _bits(vd.reshape(P, 3)[index]))
        assert torch.equal(_bits(target), _bits(images.reshape(P, 4)[index, :3]))
        full = torch.zeros((P, N), device="cuda")
        full[index] = noise
        vt = ctx.generate_rays_cam(c2w, cam, H, W, 2.0, 6.0, N, None, full.reshape(V, H, W, N))[2]
        assert torch.equal(_bits(t), _bits(vt.reshape(P, N)[index]))
        # the same pixels as a plain batch draws at these positions
        assert torch.equal(index, ctx.draw_ray_batch(images, c2w, FOCAL, 2.0, 6.0, N, seed, epoch, first, n, want_index=True)[4])
        # and the jitter of the Philox stream is the plain batch's
        assert torch.equal(_bits(ctx.draw_ray_batch(images, c2w, None, 2.0, 6.0, N, seed, epoch, first, n, noise_stream=7, camera=cam)[2]),
                           _bits(ctx.draw_ray_batch(images, c2w, FOCAL, 2.0, 6.0, N, seed, epoch, first, n, noise_stream=7)[2]))


@pytest.mark.parametrize("name,offset", CASES)
def test_projection_round_trip(ctx, scene, name, offset):
    """the ray of pixel (x, y) projects to (x, y): within 1e-4 px at s = 0.7, 3 and 9 along the ray (25x the float32 mirror's 3.9e-6),
    fisheye_wide's rays beyond 90 degrees included; depth against fp64 to 1e-5 of the point's distance"""
    cam = _camera(name, offset)
    o, d, _ = ctx.generate_rays_cam(scene["c2w"], cam, H, W, 2.0, 6.0, N, None, scene["noise"])
    view = torch.arange(V, device="cuda", dtype=torch.int32)[:, None, None].expand(V, H, W).reshape(-1)
    pixel = torch.stack(torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")[::-1], -1).float()
    behind_z = 0
    for s in (0.7, 3.0, 9.0):
        pts = o + s * d
        pix, depth, valid = cam.project(pts.reshape(-1, 3), scene["c2w"], view)
        assert pix.shape == (P, 2) and depth.shape == (P,) and valid.dtype == torch.bool and bool(valid.all())
        err = float((pix.reshape(V, H, W, 2) - pixel[None]).abs().max())
        _, depth64, _ = CR.project(CR.SETS[name], offset, scene["poses"], pts.cpu().numpy())
        derr = float(np.abs(depth.double().cpu().numpy().reshape(V, H, W) - depth64).max() / s)
        print(f"{name} offset {offset} s = {s}: round trip {err:.3g} px, depth error / distance {derr:.3g}")
        assert err <= CR.BOUND_ROUND_TRIP_PX, (s, err)
        assert derr <= CR.BOUND_DEPTH_REL, (s, derr)
        if CR.SETS[name][0] != "fisheye":
            assert float(np.abs(depth.double().cpu().numpy().reshape(V, H, W) / depth64 - 1).max()) <= CR.BOUND_DEPTH_REL
        behind_z += int((depth <= 0).sum())
        back = cam.project((o - s * d).reshape(-1, 3), scene["c2w"], view)
        if CR.SETS[name][0] != "fisheye":
            assert not bool(back[2].any()) and bool((back[1] < 0).all())                                 # behind the camera
    if name == "fisheye_wide":
        assert behind_z > 100                                                                             # rays past 90 degrees were among them
    # view = None is view 0
    p0 = cam.project((o[0] + 3.0 * d[0]).reshape(-1, 3), scene["c2w"])
    assert float((p0[0].reshape(H, W, 2) - pixel).abs().max()) <= CR.BOUND_ROUND_TRIP_PX and bool(p0[2].all())
    if CR.SETS[name][0] == "fisheye":
        centre = cam.project(scene["c2w"][:, :3, 3], scene["c2w"], torch.arange(V, dtype=torch.int32))
        assert not bool(centre[2].any())                                                                  # the camera centre has no image
        behind = cam.project(scene["c2w"][:, :3, 3] + scene["c2w"][:, :3, 2], scene["c2w"], torch.arange(V, dtype=torch.int32))
        on_axis = cam.project(scene["c2w"][:, :3, 3] - scene["c2w"][:, :3, 2], scene["c2w"], torch.arange(V, dtype=torch.int32))
        assert bool(on_axis[2].all()) and float((on_axis[0] - torch.tensor([CR.SETS[name][3] - offset, CR.SETS[name][4] - offset], device="cuda")).abs().max()) <= 1e-4
        assert float(behind[1].max()) < 0 and not bool(behind[2].any())                                  # straight behind: theta = pi
    with pytest.raises(ValueError):
        cam.project(pts.reshape(-1, 3), scene["c2w"], view + 1)                                           # a view index past the poses


def test_projection_with_a_per_view_table(ctx, scene):
    per = _per_view()
    o, d, _ = ctx.generate_rays_cam(scene["c2w"], per, H, W, 2.0, 6.0, N, None, scene["noise"])
    order = torch.randperm(P, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    view = (order // (H * W)).to(torch.int32)
    pix, depth, valid = per.project((o + 3.0 * d).reshape(P, 3)[order], scene["c2w"], view)
    want = torch.stack([(order % W).float(), ((order // W) % H).float()], -1)
    assert bool(valid.all()) and float((pix - want).abs().max()) <= CR.BOUND_ROUND_TRIP_PX
    with pytest.raises(ValueError):
        per.project(o.reshape(P, 3), scene["c2w"][:2], view.clamp(max=1))                                 # three cameras, two poses


@pytest.mark.parametrize("offset", CR.OFFSETS)
def test_opencv_rays_under_ndc_match_the_fp64_reference(ctx, scene, offset):
    """fed the kernel's own fp32 camera rays, so that only the NDC map is measured: bound 1e-5, that of
    tests/test_gpu_forward_facing.py for the same arithmetic.  forward_facing_reference.ndc_rays takes one focal length: it is asked
    once with fx for the x components and once with fy for the y components (z does not depend on it)."""
    name = "mild"
    cam = _camera(name, offset)
    fx, fy = CR.SETS[name][1:3]
    o, d, _ = ctx.generate_rays_cam(scene["c2w"], cam, H, W, 0.0, 1.0, N, None, scene["noise"])
    o64, d64 = o.double().cpu().numpy(), d.double().cpu().numpy()
    assert float(np.abs(d64[..., 2]).min()) >= 0.4                                                       # no division is ill-conditioned
    for near_plane in (1.0, 0.5):
        ox, dx, Lx = FF.ndc_rays(o64, d64, fx, W, H, near_plane)
        oy, dy, Ly = FF.ndc_rays(o64, d64, fy, W, H, near_plane)
        want_o = np.stack([ox[..., 0], oy[..., 1], ox[..., 2]], -1)
        raw = np.stack([dx[..., 0] * Lx, dy[..., 1] * Ly, dx[..., 2] * Lx], -1)
        L = np.linalg.norm(raw, axis=-1)
        no, nd, nt = ctx.generate_rays_cam(scene["c2w"], cam, H, W, 0.0, 1.0, N, _ray_model(ndc=1, ndc_near=near_plane), scene["noise"])
        errs = (_err(no, want_o), _err(nd, raw / L[..., None]), _err(nt, FF.ndc_samples(N, 0.0, 1.0, scene["noise64"], L)))
        print(f"opencv + NDC, offset {offset}, near plane {near_plane}: max |gpu - fp64| of o, d, t:", errs)
        assert max(errs) <= 1e-5, errs
        assert float((nd.norm(dim=-1) - 1).abs().max()) <= 1e-6 and float((no[..., 2] + 1).abs().max()) <= 1e-5
    # a ray batch under NDC carries the same rays
    m = _ray_model(ndc=1)
    no, nd, _ = ctx.generate_rays_cam(scene["c2w"], cam, H, W, 0.0, 1.0, N, m, scene["noise"])
    bo, bd, _, _, index = ctx.draw_ray_batch(scene["images"], scene["c2w"], None, 0.0, 1.0, N, 5, 3, 17, 700, want_index=True, ray_model=m, camera=cam)
    assert torch.equal(_bits(bo), _bits(no.reshape(P, 3)[index])) and torch.equal(_bits(bd), _bits(nd.reshape(P, 3)[index]))


def test_refusals_come_before_any_launch(ctx, scene):
    from keras_nerf_amd import _lib
    lib, c2w, images = _lib.load(), scene["c2w"], scene["images"]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shared, per = _camera("mild").device_table(), _per_view().device_table()
    fish = _camera("fisheye").device_table()
    o = torch.full((V, H, W, 3), 7.0, device="cuda"); d = torch.full_like(o, 7.0); t = torch.full((V, H, W, N), 7.0, device="cuda")
    bo = torch.full((64, 3), 7.0, device="cuda"); bd = torch.full_like(bo, 7.0); bt = torch.full((64, N), 7.0, device="cuda")
    btar = torch.full_like(bo, 7.0); bidx = torch.full((64,), 7, device="cuda", dtype=torch.int64)

    def gen(table, n_cam, model, off=0.0, ray=None, near=0.0, far=1.0):
        cs = _lib.KnerfCameraModel(model, off)
        return lib.knerf_generate_rays_cam(ctx._ctx, stream, p(c2w), p(scene["noise"]), 0, 0, V, H, W, N, p(table), n_cam, C.byref(cs), near, far,
                                           p(o), p(d), p(t), None if ray is None else C.byref(ray))

    def bat(table, n_cam, model, off=0.0, ray=None, near=0.0, far=1.0):
        cs = _lib.KnerfCameraModel(model, off)
        return lib.knerf_draw_ray_batch_cam(ctx._ctx, stream, p(images), p(c2w), V, H, W, 4, p(table), n_cam, C.byref(cs), near, far, N, 0, 0, 0, 64,
                                            None, 0, p(bo), p(bd), p(bt), p(btar), p(bidx), None if ray is None else C.byref(ray))
    for call in (gen, bat):
        for args, kw in (((fish, 1, _lib.CAMERA_FISHEYE), dict(ray=_ray_model(ndc=1))),         # FISHEYE + NDC
                         ((per, 3, _lib.CAMERA_OPENCV), dict(ray=_ray_model(ndc=1))),            # a per-view table + NDC
                         ((per, 2, _lib.CAMERA_OPENCV), {}),                                     # two cameras for three views
                         ((shared, 1, 3), {}), ((shared, 1, -1), {}),                            # a model out of range
                         ((shared, 1, _lib.CAMERA_OPENCV), dict(off=float("nan"))),
                         ((shared, 1, _lib.CAMERA_OPENCV), dict(off=float("inf"))),
                         ((None, 1, _lib.CAMERA_OPENCV), {}),
                         ((shared, 1, _lib.CAMERA_OPENCV), dict(ray=_ray_model(spacing=1))),     # what the _ext entry points refuse
                         ((shared, 1, _lib.CAMERA_OPENCV), dict(ray=_ray_model(ndc=1), near=2.0, far=6.0))):
            assert call(*args, **kw) == _lib.KNERF_ERR_INVALID, (call.__name__, args[1:], kw)
            assert ctx.lib.knerf_last_error(ctx._ctx)
    torch.cuda.synchronize()
    for x in (o, d, t, bo, bd, bt, btar):
        assert float(x.min()) == 7.0 and float(x.max()) == 7.0                                   # nothing was launched
    assert int(bidx.min()) == 7 and int(bidx.max()) == 7
    # the same arguments without the fault go through
    assert gen(shared, 1, _lib.CAMERA_OPENCV) == 0 and bat(per, 3, _lib.CAMERA_OPENCV) == 0
    torch.cuda.synchronize()
    assert float(t.max()) <= 1.0 and float(bt.max()) <= 1.0 and int(bidx.max()) < P
    # the Python surface says the same before it calls
    with pytest.raises(Exception):
        ctx.generate_rays_cam(c2w, _per_view(), H, W, 0.0, 1.0, N, _ray_model(ndc=1), scene["noise"])
    with pytest.raises(Exception):
        ctx.draw_ray_batch(images, c2w, None, 0.0, 1.0, N, 0, 0, 0, 64, ray_model=_ray_model(ndc=1), camera=_camera("fisheye"))
    with pytest.raises(Exception):
        ctx.draw_ray_batch(images, c2w, None, 2.0, 6.0, N, 0, 0, 0, 64, camera=_per_view().select([0, 1]))


def _write_scene(root, n_views=6):
    """a transforms_*.json scene of 12 x 20 images: the train file states one camera per frame (the strong set, with a focal length
    that varies from frame to frame), the val and test files one camera at top level (the mild set at twice the size)"""
    from PIL import Image
    rng = np.random.default_rng(4)
    poses = FF.random_poses(n_views, seed=11).astype(np.float64)
    poses[:, :3, 3] += poses[:, :3, 2] * 4.0                                           # cameras 4 units back along their own axes
    _, fx, fy, cx, cy, (k1, k2, p1, p2, k3) = CR.SETS["strong"]
    _, mfx, mfy, mcx, mcy, (mk1, mk2, mp1, mp2, mk3) = CR.SETS["mild"]
    for subset, idx in (("train", range(n_views)), ("val", range(2)), ("test", range(2))):
        (root / subset).mkdir(parents=True, exist_ok=True)
        frames = []
        for i in idx:
            Image.fromarray(rng.integers(0, 256, (H, W, 4), dtype=np.uint8), "RGBA").save(root / subset / f"r_{i}.png")
            fr = dict(file_path=f"./{subset}/r_{i}", transform_matrix=poses[i].tolist())
            if subset == "train":
                fr.update(fl_x=fx + 0.25 * i, fl_y=fy + 0.25 * i, cx=cx, cy=cy, k1=k1, k2=k2, p1=p1, p2=p2, k3=k3)
            frames.append(fr)
        cfg = dict(frames=frames, w=W, h=H, camera_model="OPENCV")
        if subset != "train":
            cfg.update(w=2 * W, h=2 * H, fl_x=2 * mfx, fl_y=2 * mfy, cx=2 * mcx, cy=2 * mcy, k1=mk1, k2=mk2, p1=mp1, p2=mp2, k3=mk3)
        (root / f"transforms_{subset}.json").write_text(json.dumps(cfg))
    return str(root), poses


def test_transforms_scene_with_distortion_keys_to_fit(tmp_path):
    """the data layer and both training modes on 12 x 20 images; no assertion that the loss falls"""
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.model.nerf.nerf import NeRF
    root, poses = _write_scene(tmp_path / "scene")
    n_coarse = 32
    load = lambda: DatasetLoader(root).load_dataset(1, W, H, 2.0, 6.0, n_coarse)
    ld = DatasetLoader(root)
    train, val, test = ld.load_dataset(1, W, H, 2.0, 6.0, n_coarse)
    assert [c.n_cameras for c in ld.cameras] == [6, 1, 1] and all(c.model == "opencv" and c.pixel_offset == 0.5 for c in ld.cameras)
    assert np.array_equal(ld.cameras[1].table(), _camera("mild", 0.5).table())
    nerf = NeRF(n_coarse=n_coarse, n_fine=32, n_layers=4, dense_units=64, skip_layer=2, seed=1)
    nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=1, image_height=H, image_width=W, ray_chunks=240)
    before = [nerf.coarse.get_flat_weights().copy(), nerf.fine.get_flat_weights().copy()]
    seen = 0
    for img, (o, d, t) in train:                                   # every view once: its rays are those of its own camera row
        assert img.shape == (1, H, W, 4) and o.shape == d.shape == (1, H, W, 3) and t.shape == (1, H, W, n_coarse)
        v = int(np.argmin([np.abs(poses[i][:3, 3].astype(np.float32) - o[0, 0, 0].cpu().numpy()).max() for i in range(6)]))
        want = CR.camera_rays(("opencv", 11.0 + 0.25 * v, 10.5 + 0.25 * v) + CR.SETS["strong"][3:], 0.5, poses[v:v + 1].astype(np.float32))[1]
        assert _err(d, want) <= CR.BOUND_DIRECTION
        seen += 1
    assert seen == 6
    h = nerf.fit(train.take(2), epochs=1, verbose=0)
    assert h.params["steps"] == 2 and all(len(v) == 1 and np.all(np.isfinite(v)) for v in h.history.values()), h.history
    mid = [nerf.coarse.get_flat_weights().copy(), nerf.fine.get_flat_weights().copy()]
    assert all(not np.array_equal(a, b) for a, b in zip(before, mid))
    rb = train.ray_batches(240, seed=2, steps_per_epoch=2)
    assert rb.ray_model() is None
    h = nerf.fit(rb, epochs=1, verbose=0)
    assert h.params["steps"] == 2 and all(np.all(np.isfinite(v)) for v in h.history.values()), h.history
    assert all(not np.array_equal(a, b) for a, b in zip(mid, [nerf.coarse.get_flat_weights(), nerf.fine.get_flat_weights()]))
    logs = nerf.test_step(next(iter(val)))
    assert all(np.isfinite(float(v)) for v in logs.values()), dict(logs)
    nerf._ctx.poll_nonfinite(wait=True)
    # a camera provider that returns the dataset's own matrices changes nothing, and last_view names each ray's camera
    plain, hooked = (load()[0].ray_batches(240, seed=2, steps_per_epoch=2) for _ in range(2))
    cams = hooked._resident_all()[1]
    hooked.set_cameras(lambda: cams)
    n = 0
    for (ta, (oa, da, tsa)), (tb, (ob, db, tsb)) in zip(plain, hooked):
        assert _same((ta, oa, da, tsa), (tb, ob, db, tsb))
        assert hooked.last_view.dtype == torch.int32 and torch.equal(ob, cams[hooked.last_view.long(), :3, 3])
        perm, first, count = hooked.last_draw
        index = ctx_free_index(hooked, perm, first, count)
        assert torch.equal(hooked.last_view.to(torch.int64), index // (H * W))
        # and the rays are those of the view kernel under the per-view table
        vo, vd, _ = hooked._rg(cams)
        assert torch.equal(_bits(db), _bits(vd.reshape(-1, 3)[index]))
        n += 1
    assert n == 2 and plain.last_view is None


def ctx_free_index(batches, perm, first, count):
    """the pixels a plain batch draws at these positions (the permutation does not depend on the camera)"""
    from keras_nerf_amd.runtime import draw_ray_batch
    return draw_ray_batch(*batches._resident_all(), FOCAL, 2.0, 6.0, 4, batches.seed, perm, first, count, want_index=True)[4]
