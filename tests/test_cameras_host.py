"""Camera models without a GPU: the float32 mirror of the kernels' arithmetic against the fp64 restatements
(tests/camera_reference.py), the properties of the shared camera sets that tests/test_gpu_cameras.py relies on, CameraModel, the ctypes
surface, and the two loaders that state cameras (transforms.json keys, COLMAP's text model).

The GPU bounds (camera_reference.BOUND_*) sit well above what fp32 does to these cameras: the mirror must stay within a fifth of each,
for every set and both pixel offsets.  Depth is compared relative to the point's distance from the camera: it is a sum of three
products of that magnitude and crosses zero at 90 degrees off the axis of a fisheye, where an error relative to itself has no bound."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import camera_reference as R
from tests import forward_facing_reference as FF

H, W = R.H, R.W
CASES = [(name, off) for name in R.SETS for off in R.OFFSETS]


@pytest.fixture(scope="module")
def poses():
    return FF.random_poses(R.V, FF.GPU_POSE_SEED)


def _model(name, offset=0.0):
    from keras_nerf_amd.data.cameras import CameraModel
    model, fx, fy, cx, cy, c = R.SETS[name]
    return CameraModel(model, fx, fy, cx, cy, c, pixel_offset=offset)


@pytest.mark.parametrize("name,offset", CASES)
def test_the_float32_mirror_stays_within_a_fifth_of_every_gpu_bound(name, offset, poses):
    cam = R.SETS[name]
    o64, d64 = R.camera_rays(cam, offset, poses)
    o32, d32 = R.camera_rays32(cam, offset, poses)
    assert np.array_equal(o32, np.broadcast_to(poses[:, None, None, :3, 3], o32.shape)) and np.array_equal(o32.astype(np.float64), o64)
    err_d = float(np.abs(d32 - d64).max())
    err_unit = float(np.abs(np.linalg.norm(d32.astype(np.float64), axis=-1) - 1).max())
    pixel = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).astype(np.float64)[None]
    err_px = err_depth = 0.0
    for s in (0.7, 3.0, 9.0):
        p = o32 + np.float32(s) * d32
        pix, depth, valid = R.project32(cam, offset, poses, p)
        _, depth64, valid64 = R.project(cam, offset, poses, p)
        assert valid.all() and valid64.all()
        err_px = max(err_px, float(np.abs(pix - pixel).max()))
        err_depth = max(err_depth, float(np.abs(depth - depth64).max() / s))
    print(f"{name} offset {offset}: direction {err_d:.3g}, unit {err_unit:.3g}, round trip {err_px:.3g} px, depth {err_depth:.3g}")
    assert err_d <= R.BOUND_DIRECTION / 5 and err_unit <= R.BOUND_UNIT / 5
    assert err_px <= R.BOUND_ROUND_TRIP_PX / 5 and err_depth <= R.BOUND_DEPTH_REL / 5


def test_the_stated_figures_of_the_distorted_sets_hold(poses):
    """8 float32 Newton steps within 3.4e-7 of the 30-step fp64 solve (normalised coordinates), the rotated unit direction within
    1.6e-7 and the ray -> point -> pixel round trip within 3.9e-6 px for the sets mild and strong; two steps miss the GPU bound on the
    direction a hundredfold on the strong set, so the step count is visible to it"""
    worst = dict(norm=0.0, direction=0.0, px=0.0)
    pixel = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).astype(np.float64)[None]
    for name in ("mild", "strong"):
        cam = R.SETS[name]
        for offset in R.OFFSETS:
            _, _, xu, yu = R.normalised32(cam, offset)
            X, Y = R.undistort(cam[5], *R.normalised(cam, offset))
            worst["norm"] = max(worst["norm"], float(np.abs(xu - X).max()), float(np.abs(yu - Y).max()))
            o32, d32 = R.camera_rays32(cam, offset, poses)
            worst["direction"] = max(worst["direction"], float(np.abs(d32 - R.camera_rays(cam, offset, poses)[1]).max()))
            for s in (0.7, 3.0, 9.0):
                worst["px"] = max(worst["px"], float(np.abs(R.project32(cam, offset, poses, o32 + np.float32(s) * d32)[0] - pixel).max()))
    print(worst)
    assert worst["norm"] <= 3.4e-7 and worst["direction"] <= 1.6e-7 and worst["px"] <= 3.9e-6
    cam = R.SETS["strong"]
    two = R.camera_rays32(cam, 0.0, poses, steps=2)[1]
    assert float(np.abs(two - R.camera_rays(cam, 0.0, poses)[1]).max()) > 100 * R.BOUND_DIRECTION


def test_every_set_is_invertible_over_the_whole_grid():
    """the determinant of the distortion Jacobian (central differences in fp64, not the analytic one under test) along the sweep
    from the principal point to EVERY pixel's solution, and d theta_d / d theta for the fisheyes: minima 0.82 (mild), 0.23 (strong),
    0.86 (fisheye), 0.88 (fisheye_wide); and the 30-step solution reproduces the pixel, so no pixel is excluded anywhere"""
    want = {"mild": 0.82, "strong": 0.23, "fisheye": 0.86, "fisheye_wide": 0.88}
    s = np.linspace(0.0, 1.0, 65)[:, None, None]
    for name, floor in want.items():
        cam = R.SETS[name]
        low = 1.0
        for offset in R.OFFSETS:
            xn, yn = R.normalised(cam, offset)
            if cam[0] == "opencv":
                xu, yu = R.undistort(cam[5], xn, yn)
                fx, fy = R.distort(cam[5], xu, yu)
                assert float(np.hypot(fx - xn, fy - yn).max()) <= 1e-12
                j = R.distort_jacobian(cam[5], s * xu[None], s * yu[None])
                low = min(low, float((j[..., 0, 0] * j[..., 1, 1] - j[..., 0, 1] * j[..., 1, 0]).min()))
            else:
                thd = np.hypot(xn, yn)
                th = R.fisheye_theta(cam[5], thd)
                assert float(np.abs(R.fisheye_theta_d(cam[5], th) - thd).max()) <= 1e-12 and float(th.max()) < np.pi
                low = min(low, float(R.fisheye_slope(cam[5], s * th[None]).min()))
        print(name, "minimum", low)
        assert floor - 0.005 <= low <= floor + 0.01, (name, low)
    th = R.fisheye_theta(R.SETS["fisheye_wide"][5], np.hypot(*R.normalised(R.SETS["fisheye_wide"], 0.0)))
    assert np.degrees(th.max()) > 145        # the wide set does look past 90 degrees
    # CameraModel.check_invertible agrees (it sweeps to the border pixels only, so its minimum is no smaller)
    for name, floor in want.items():
        for offset in R.OFFSETS:
            got = _model(name, offset).check_invertible(W, H)
            assert got["min_det"] >= floor - 0.005 and got["max_residual"] <= 1e-12
    assert _model("intrinsics").check_invertible(W, H)["min_det"] == 1.0


def test_check_invertible_refuses_what_the_kernels_cannot():
    from keras_nerf_amd.data.cameras import CameraModel
    _, fx, fy, cx, cy, _ = R.SETS["strong"]
    with pytest.raises(ValueError, match="fold|invertible"):
        CameraModel("opencv", fx, fy, cx, cy, (-0.6,)).check_invertible(W, H)
    assert CameraModel("opencv", fx, fy, cx, cy, (-0.1,)).check_invertible(W, H)["min_det"] > 0        # a weaker lens of the same kind passes
    with pytest.raises(ValueError, match="fold|invertible|pi"):
        CameraModel("fisheye", 2.0, 2.0, cx, cy, (-0.2,)).check_invertible(W, H)
    for bad in (dict(fx=0.0), dict(fx=-3.0), dict(fy=0.0), dict(fx=float("nan")), dict(cx=float("inf")), dict(distortion=(float("nan"),)),
                dict(pixel_offset=float("nan"))):
        kw = dict(model="opencv", fx=fx, fy=fy, cx=cx, cy=cy, distortion=(0.01,), pixel_offset=0.0)
        kw.update(bad)
        with pytest.raises(ValueError, match="finite|positive"):
            CameraModel(**kw).check_invertible(W, H)
    with pytest.raises(ValueError):
        CameraModel("pinhole", [1.0, -1.0], 1.0, 0.0, 0.0).check_invertible(W, H)   # one bad row of a per-view table
    with pytest.raises(ValueError):
        CameraModel("plenoptic", 1, 1, 0, 0)
    with pytest.raises(ValueError):
        CameraModel("fisheye", 1, 1, 0, 0, (0, 0, 0, 0, 0))                        # five coefficients for a model of four
    with pytest.raises(ValueError):
        CameraModel("opencv", [1, 2], [1, 2, 3], 0, 0)                             # per-view lengths that disagree


def test_table_layout_scaled_select_and_from_focal():
    from keras_nerf_amd import _lib
    from keras_nerf_amd.data.cameras import CameraModel
    cam = _model("mild", 0.5)
    t = cam.table()
    assert t.dtype == np.float32 and t.shape == (1, _lib.CAMERA_ROW) == (1, 12) and cam.n_cameras == 1
    assert np.array_equal(t[0], np.array([18, 17, 10.3, 5.6, -0.12, 0.03, 0.002, -0.003, -0.004, 0, 0, 0], np.float32))
    assert np.array_equal(_model("fisheye").table()[0], np.array([7, 6.8, 9.6, 6.2, -0.04, 0.01, -0.003, 0.0005, 0, 0, 0, 0], np.float32))
    assert np.array_equal(_model("intrinsics").table()[0, 4:], np.zeros(8, np.float32))
    s = cam.scaled(2.0, 0.5).table()[0]
    assert np.array_equal(s[:4], np.array([36, 8.5, 20.6, 2.8], np.float32)) and np.array_equal(s[4:], t[0, 4:])
    assert cam.scaled(2.0, 0.5).pixel_offset == 0.5 and cam.scaled(2.0, 0.5).model == "opencv"
    assert cam.select([2, 0]) is cam                                               # a shared camera stays shared
    per = CameraModel("opencv", [18, 11, 12], [17, 10.5, 12], 10.0, [5.6, 6.3, 6.0], [[-0.12, 0.03], [-0.25, 0.07], [0, 0]], 0.5)
    assert per.n_cameras == 3 and per.table().shape == (3, 12) and np.array_equal(per.table()[:, 2], np.full(3, 10, np.float32))
    sel = per.select([2, 0])
    assert sel.n_cameras == 2 and np.array_equal(sel.table(), per.table()[[2, 0]]) and sel.pixel_offset == 0.5
    with pytest.raises(ValueError):
        per.select([3])
    plain = CameraModel.from_focal(18.0, W, H)
    assert plain.model == "pinhole" and plain.pixel_offset == 0.0
    assert np.array_equal(plain.table()[0, :4], np.array([18, 18, W * 0.5, H * 0.5], np.float32))


def test_the_ctypes_surface_matches_the_header():
    from keras_nerf_amd import _lib, build
    assert C.sizeof(_lib.KnerfCameraModel) == 8 and C.sizeof(_lib.KnerfRayModel) == 12
    assert [(n, t) for n, t in _lib.KnerfCameraModel._fields_] == [("model", C.c_int32), ("pixel_offset", C.c_float)]
    assert _lib.KnerfCameraModel.pixel_offset.offset == 4
    assert (_lib.CAMERA_PINHOLE, _lib.CAMERA_OPENCV, _lib.CAMERA_FISHEYE) == (0, 1, 2)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "knerf.h")).read()
    assert "enum { KNERF_CAMERA_PINHOLE = 0, KNERF_CAMERA_OPENCV = 1, KNERF_CAMERA_FISHEYE = 2 };" in hdr
    lib = _lib.load()
    for name in ("knerf_generate_rays_cam", "knerf_draw_ray_batch_cam", "knerf_project_points"):
        assert name in _lib.SIGNATURES and f"int {name}(" in hdr and hasattr(lib, name)
    # focal (one float) gave way to (intrinsics, n_cameras, camera): everything else is the _ext signature
    for cam, ext, at in (("knerf_generate_rays_cam", "knerf_generate_rays_ext", 10), ("knerf_draw_ray_batch_cam", "knerf_draw_ray_batch_ext", 8)):
        a, b = _lib.SIGNATURES[cam][1], _lib.SIGNATURES[ext][1]
        assert b[at] is C.c_float and a[:at] == b[:at] and a[at + 3:] == b[at + 1:]
        assert a[at:at + 3] == [C.c_void_p, C.c_int, C.POINTER(_lib.KnerfCameraModel)]
    assert "rays_cam.hip" in build.SOURCES and "rays_cam.hip" in build.NO_SPILL and "rays_cam.hip" not in build.SLICED
    assert "rays_cam.h" in build.HEADERS and not set(build.KERNEL_FILES) & {"rays_cam.hip", "rays_cam.h", "rays_ext.h", "rays.h"}


def test_the_entry_points_refuse_bad_cameras_before_any_launch():
    """KNERF_ERR_INVALID from the argument checks alone: no device is needed, the pointers are never read"""
    from keras_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)
    cam = lambda model=0, off=0.0: C.byref(_lib.KnerfCameraModel(model, off))
    ray = lambda ndc=0, spacing=0: C.byref(_lib.KnerfRayModel(ndc, spacing, 1.0))
    gen = lambda n_cam, c, m, near=0.0, far=1.0, intr=p: lib.knerf_generate_rays_cam(None, None, p, None, 0, 0, 3, H, W, 8, intr, n_cam, c, near,
                                                                                    far, p, p, p, m)
    bat = lambda n_cam, c, m, intr=p: lib.knerf_draw_ray_batch_cam(None, None, p, p, 3, H, W, 4, intr, n_cam, c, 0.0, 1.0, 8, 0, 0, 0, 16, None, 0,
                                                                    p, p, p, p, None, m)
    for call in (gen, bat):
        assert call(1, cam(2), ray(ndc=1)) == _lib.KNERF_ERR_INVALID and b"fisheye" in lib.knerf_last_error(None)
        assert call(3, cam(1), ray(ndc=1)) == _lib.KNERF_ERR_INVALID and b"n_cameras" in lib.knerf_last_error(None)
        assert call(2, cam(1), None) == _lib.KNERF_ERR_INVALID and b"n_cameras" in lib.knerf_last_error(None)
        assert call(0, cam(0), None) == _lib.KNERF_ERR_INVALID
        for model in (-1, 3):
            assert call(1, cam(model), None) == _lib.KNERF_ERR_INVALID and b"camera model" in lib.knerf_last_error(None)
        for off in (float("nan"), float("inf")):
            assert call(1, cam(0, off), None) == _lib.KNERF_ERR_INVALID and b"pixel_offset" in lib.knerf_last_error(None)
        assert call(1, None, None) == _lib.KNERF_ERR_INVALID and call(1, cam(0), None, intr=None) == _lib.KNERF_ERR_INVALID
        assert call(1, cam(1), ray(ndc=1, spacing=1)) == _lib.KNERF_ERR_INVALID            # what the _ext entry points refuse
    assert gen(1, cam(1), ray(spacing=1), near=0.0, far=6.0) == _lib.KNERF_ERR_INVALID      # disparity spacing needs near > 0
    assert gen(1, cam(0), ray(ndc=1), near=2.0, far=6.0) == _lib.KNERF_ERR_INVALID
    proj = lambda n_cam, c, n=5, pts=p: lib.knerf_project_points(None, pts, None, p, p, n_cam, c, n, p, p, p)
    assert proj(1, cam(3)) == _lib.KNERF_ERR_INVALID and proj(0, cam(0)) == _lib.KNERF_ERR_INVALID and proj(1, cam(0), n=0) == _lib.KNERF_ERR_INVALID
    assert proj(1, cam(0, float("nan"))) == _lib.KNERF_ERR_INVALID and proj(1, None) == _lib.KNERF_ERR_INVALID
    assert proj(1, cam(0), pts=None) == _lib.KNERF_ERR_INVALID


# ---- transforms.json
def _frames(n, extra=lambda i: {}):
    return [dict(file_path=f"./train/r_{i}", transform_matrix=np.eye(4).tolist(), **extra(i)) for i in range(n)]


def test_transforms_keys_at_top_level_per_frame_and_absent(tmp_path):
    from keras_nerf_amd.data.loader import DatasetLoader, camera_from_transforms
    top = dict(fl_x=36.0, fl_y=34.0, cx=20.6, cy=11.2, w=40, h=24, k1=-0.12, k2=0.03, p1=0.002, p2=-0.003, k3=-0.004, camera_model="OPENCV",
               frames=_frames(3))
    cam = camera_from_transforms(top, W, H)
    assert cam.model == "opencv" and cam.n_cameras == 1 and cam.pixel_offset == 0.5
    assert np.array_equal(cam.table(), _model("mild", 0.5).table())                      # 40 x 24 -> 20 x 12: the mild set
    fish = camera_from_transforms(dict(top, camera_model="OPENCV_FISHEYE", k4=0.001), W, H)
    assert fish.model == "fisheye" and np.allclose(fish.table()[0, 4:8], [-0.12, 0.03, -0.004, 0.001])
    assert camera_from_transforms(dict(fl_x=36.0, w=40, h=24, frames=_frames(2)), W, H).model == "pinhole"
    assert np.array_equal(camera_from_transforms(dict(fl_x=36.0, w=40, h=24, frames=_frames(2)), W, H).table()[0, :4], np.array([18, 18, 10, 6], np.float32))
    per = dict(w=40, h=24, cx=20.0, frames=_frames(3, lambda i: dict(fl_x=30.0 + i, fl_y=31.0 + i, cy=11.0 + i, k1=0.01 * i)))
    cam = camera_from_transforms(per, W, H)
    assert cam.model == "opencv" and cam.n_cameras == 3                                  # frame 0 has no distortion: promoted
    assert np.allclose(cam.table()[:, 0], [15, 15.5, 16]) and np.allclose(cam.table()[:, 3], [5.5, 6, 6.5]) and np.allclose(cam.table()[:, 4], [0, 0.01, 0.02])
    assert np.allclose(cam.table()[:, 2], 10.0)
    mixed = dict(w=40, h=24, frames=_frames(2, lambda i: dict(fl_x=30.0, k1=0.01, camera_model=("OPENCV", "OPENCV_FISHEYE")[i])))
    with pytest.raises(ValueError, match="mixes"):
        camera_from_transforms(mixed, W, H)
    with pytest.raises(ValueError, match="not supported"):
        camera_from_transforms(dict(top, camera_model="EQUIRECTANGULAR"), W, H)
    assert camera_from_transforms(dict(camera_angle_x=0.69, frames=_frames(2)), W, H) is None
    # through the loader: a calibrated train file beside plain val / test files
    root = tmp_path / "scene"
    root.mkdir()
    for subset, cfg in (("train", top), ("val", dict(camera_angle_x=0.69, frames=_frames(2))), ("test", dict(camera_angle_x=0.69, frames=_frames(2)))):
        (root / f"transforms_{subset}.json").write_text(json.dumps(cfg))
    ld = DatasetLoader(str(root))
    train, val, test = ld.load_dataset(1, W, H, 2.0, 6.0, 8)
    assert ld.cameras[0].model == "opencv" and ld.cameras[1] is None and ld.cameras[2] is None
    assert train.image_loader.output_size == (H, W) and val.image_loader.output_size == (W, H)      # the plain files: as before
    assert len(train) == 3 and train.image_paths[0].endswith("r_0.png")
    bad = dict(top, k1=-5.0)
    (root / "transforms_train.json").write_text(json.dumps(bad))
    with pytest.raises(ValueError, match="fold|invertible"):
        DatasetLoader(str(root)).load_dataset(1, W, H, 2.0, 6.0, 8)


# ---- COLMAP's text model
def _write_colmap(root, cameras, images, points=None, binary=False):
    model = root / "sparse" / "0"
    model.mkdir(parents=True)
    if binary:
        (model / "cameras.bin").write_bytes(b"\0" * 8)
        return str(root)
    (model / "cameras.txt").write_text("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n" + "\n".join(cameras) + "\n")
    lines = ["# Image list with two lines of data per image:", "#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME", "#   POINTS2D[] as (X, Y, POINT3D_ID)"]
    for k, im in enumerate(images):
        lines += [im, "" if k % 2 else "1.5 2.5 -1 3.5 4.5 7"]                      # the second line may be empty
    (model / "images.txt").write_text("\n".join(lines) + "\n")
    if points is not None:
        (model / "points3D.txt").write_text("# 3D point list\n" + "\n".join(points) + "\n")
    return str(root)


def test_colmap_pose_from_a_hand_computed_quaternion(tmp_path):
    """a camera turned 90 degrees about the world's y axis: q = (cos 45, 0, sin 45, 0) maps world to camera as x_cam = R x + t with
    R = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]; t = (1, 2, 3).  Then the centre is -R^T t = (3, -2, -1), the camera's right axis is the
    first row of R, (0, 0, 1); its down axis (0, 1, 0), so up is (0, -1, 0); its forward axis (-1, 0, 0), so backwards is (1, 0, 0)."""
    from keras_nerf_amd.data.colmap import ColmapDatasetLoader, colmap_to_c2w
    r = np.sqrt(0.5)
    want = np.array([[0, 0, 1, 3], [0, -1, 0, -2], [1, 0, 0, -1], [0, 0, 0, 1]], np.float64)
    assert np.allclose(colmap_to_c2w((r, 0, r, 0), (1, 2, 3)), want, atol=1e-15)
    assert np.allclose(colmap_to_c2w((2 * r, 0, 2 * r, 0), (1, 2, 3)), want, atol=1e-15)            # normalised on the way
    assert np.allclose(colmap_to_c2w((1, 0, 0, 0), (0, 0, 0)), np.diag([1.0, -1.0, -1.0, 1.0]))
    root = _write_colmap(tmp_path / "a", ["1 PINHOLE 40 24 36 34 20.6 11.2"],
                         [f"{i + 1} {r} 0 {r} 0 1 2 3 1 img_{2 - i}.png" for i in range(3)])
    ld = ColmapDatasetLoader(root, holdout=2)
    train, val, test = ld.load_dataset(1, W, H, 2.0, 6.0, 8)
    assert [os.path.basename(q) for q in ld.image_paths] == ["img_0.png", "img_1.png", "img_2.png"]       # name order
    assert np.allclose(ld.poses, want[None]) and ld.bounds is None
    assert ld.camera.model == "pinhole" and ld.camera.n_cameras == 3 and ld.camera.pixel_offset == 0.5
    assert np.allclose(ld.camera.table()[:, :4], [[18, 17, 10.3, 5.6]] * 3)
    assert len(train.image_paths) == 1 and len(val.image_paths) == 2 and val.image_paths == test.image_paths
    assert train.camera_params[0].dtype == np.float32 and train.image_loader.output_size == (H, W)


def test_colmap_parameter_order_promotion_and_refusals(tmp_path):
    from keras_nerf_amd.data.colmap import ColmapDatasetLoader, read_cameras
    cams = ["1 SIMPLE_PINHOLE 20 12 18 10.3 5.6", "2 PINHOLE 20 12 18 17 10.3 5.6", "3 SIMPLE_RADIAL 20 12 18 10.3 5.6 -0.12",
            "4 RADIAL 20 12 18 10.3 5.6 -0.12 0.03", "5 OPENCV 40 24 36 34 20.6 11.2 -0.12 0.03 0.002 -0.003",
            "6 OPENCV_FISHEYE 20 12 7 6.8 9.6 6.2 -0.04 0.01 -0.003 0.0005"]
    ident = lambda i, cam: f"{i} 1 0 0 0 0 0 0 {cam} v{i}.png"
    root = _write_colmap(tmp_path / "a", cams, [ident(i, i) for i in range(1, 6)])
    got = read_cameras(os.path.join(root, "sparse", "0", "cameras.txt"))
    assert got[1] == ("pinhole", 20, 12, 18.0, 18.0, 10.3, 5.6, ()) and got[2] == ("pinhole", 20, 12, 18.0, 17.0, 10.3, 5.6, ())
    assert got[3][3:] == (18.0, 18.0, 10.3, 5.6, (-0.12, 0.0, 0.0, 0.0, 0.0)) and got[4][7] == (-0.12, 0.03, 0.0, 0.0, 0.0)
    assert got[5][7] == (-0.12, 0.03, 0.002, -0.003, 0.0) and got[6] == ("fisheye", 20, 12, 7.0, 6.8, 9.6, 6.2, (-0.04, 0.01, -0.003, 0.0005))
    ld = ColmapDatasetLoader(root)
    ld.load_dataset(1, W, H, 2.0, 6.0, 8)
    t = ld.camera.table()
    assert ld.camera.model == "opencv" and t.shape == (5, 12)                       # pinhole cameras promoted, zero coefficients
    assert np.array_equal(t[0], np.array([18, 18, 10.3, 5.6] + [0] * 8, np.float32)) and np.array_equal(t[1, :4], np.array([18, 17, 10.3, 5.6], np.float32))
    assert np.array_equal(t[2, 4:9], np.array([-0.12, 0, 0, 0, 0], np.float32)) and np.array_equal(t[3, 4:9], np.array([-0.12, 0.03, 0, 0, 0], np.float32))
    assert np.array_equal(t[4], np.array([18, 17, 10.3, 5.6, -0.12, 0.03, 0.002, -0.003, 0, 0, 0, 0], np.float32))      # scaled per camera
    root = _write_colmap(tmp_path / "b", cams, [ident(1, 1), ident(2, 6)])
    ld = ColmapDatasetLoader(root, holdout=2)
    ld.load_dataset(1, W, H, 2.0, 6.0, 8)
    assert ld.camera.model == "fisheye" and np.array_equal(ld.camera.table()[:, 4:8], np.array([[0, 0, 0, 0], [-0.04, 0.01, -0.003, 0.0005]], np.float32))
    with pytest.raises(ValueError, match="mixes"):
        ColmapDatasetLoader(_write_colmap(tmp_path / "c", cams, [ident(1, 3), ident(2, 6)])).load_dataset(1, W, H, 2.0, 6.0, 8)
    with pytest.raises(ValueError, match="binary.*text|text"):
        ColmapDatasetLoader(_write_colmap(tmp_path / "d", [], [], binary=True)).load_dataset(1, W, H, 2.0, 6.0, 8)
    with pytest.raises(ValueError, match="FULL_OPENCV"):
        ColmapDatasetLoader(_write_colmap(tmp_path / "e", ["1 FULL_OPENCV 20 12 18 17 10.3 5.6 0 0 0 0 0 0 0 0"], [ident(1, 1)])).load_dataset(1, W, H, 2.0, 6.0, 8)
    with pytest.raises(ValueError, match="parameters"):
        ColmapDatasetLoader(_write_colmap(tmp_path / "f", ["1 PINHOLE 20 12 18 10.3 5.6"], [ident(1, 1)])).load_dataset(1, W, H, 2.0, 6.0, 8)
    with pytest.raises(ValueError, match="fold|invertible"):
        ColmapDatasetLoader(_write_colmap(tmp_path / "g", ["1 SIMPLE_RADIAL 20 12 11 9.4 6.3 -0.6"], [ident(1, 1)])).load_dataset(1, W, H, 2.0, 6.0, 8)


def test_colmap_near_far_from_three_points(tmp_path):
    """identity pose: depth = z.  Image 1 observes the points at z = 2, 4, 10, image 2 those at 4 and 10; the 0.1 / 99.9 percentiles
    interpolate linearly between the order statistics"""
    from keras_nerf_amd.data.colmap import ColmapDatasetLoader
    pts = ["1 0.1 0.2 2.0 255 0 0 0.5 1 0", "2 -0.3 0.1 4.0 0 255 0 0.5 1 1 2 0", "3 0.5 -0.4 10.0 0 0 255 0.5 2 1 1 2"]
    images = ["1 1 0 0 0 0 0 0 1 a.png", "2 1 0 0 0 0 0 0 1 b.png"]
    ld = ColmapDatasetLoader(_write_colmap(tmp_path / "a", ["1 PINHOLE 20 12 18 17 10.3 5.6"], images, pts), holdout=2)
    ld.load_dataset(1, W, H, 2.0, 6.0, 8)
    want = np.array([np.percentile([2.0, 4.0, 10.0], [0.1, 99.9]), np.percentile([4.0, 10.0], [0.1, 99.9])])
    assert np.allclose(ld.bounds, want, rtol=0, atol=1e-12) and np.allclose(want[0], [2.004, 9.988])
    # a camera moved back by 1 along its axis sees everything one unit deeper: t_z = +1 in world-to-camera terms
    ld = ColmapDatasetLoader(_write_colmap(tmp_path / "b", ["1 PINHOLE 20 12 18 17 10.3 5.6"], ["1 1 0 0 0 0 0 1 1 a.png", images[1]], pts), holdout=2)
    ld.load_dataset(1, W, H, 2.0, 6.0, 8)
    assert np.allclose(ld.bounds[0], want[0] + 1.0) and np.allclose(ld.bounds[1], want[1])
    # bd_factor: the nearest bound lands at 1 / bd_factor, translations scale with it
    ld = ColmapDatasetLoader(_write_colmap(tmp_path / "c", ["1 PINHOLE 20 12 18 17 10.3 5.6"], ["1 1 0 0 0 0 0 1 1 a.png", images[1]], pts), holdout=2,
                             bd_factor=0.75)
    ld.load_dataset(1, W, H, 2.0, 6.0, 8)
    assert np.isclose(ld.bounds.min(), 1 / 0.75) and np.allclose(ld.poses[0, :3, 3], np.array([0, 0, -1.0]) / (3.004 * 0.75))       # the centre is -R^T t
    with pytest.raises(ValueError, match="points3D"):
        ColmapDatasetLoader(_write_colmap(tmp_path / "d", ["1 PINHOLE 20 12 18 17 10.3 5.6"], images), bd_factor=0.75).load_dataset(1, W, H, 2.0, 6.0, 8)
