"""Forward-facing scenes, the host side (no GPU): the fp64 NDC reference on its own terms, the LLFF loader on a directory written
here, the spiral render path, and the argument checks of RaysGenerator (tests/README_forward_facing.md)."""
import os

import numpy as np
import pytest

from keras_nerf_amd.data.llff import LLFFDatasetLoader
from keras_nerf_amd.data.utils import poses_avg, recenter_poses, render_path_spiral
from tests import forward_facing_reference as R

H, W, FOCAL = 12, 20, 18.0


def _pinhole(c2w, focal=FOCAL):
    """fp64 pinhole rays of every pixel corner: o, d [V,H,W,3]"""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    cam = np.stack([(x - W / 2) / focal, -(y - H / 2) / focal, -np.ones_like(x)], -1)
    d = np.einsum("hwk,vrk->vhwr", cam, np.asarray(c2w, np.float64)[:, :3, :3])
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(np.asarray(c2w, np.float64)[:, None, None, :3, 3], d.shape)
    return o, d


def test_the_ndc_reference_is_right_on_its_own_terms():
    o, d = _pinhole(R.random_poses(3, seed=R.GPU_POSE_SEED))
    for n in (1.0, 0.5):
        o2, d2, L = R.ndc_rays(o, d, FOCAL, W, H, n)
        assert np.abs(o2[..., 2] + 1.0).max() <= 1e-12
        assert np.abs((o2 + L[..., None] * d2)[..., 2] - 1.0).max() <= 1e-12
        assert np.abs(np.linalg.norm(d2, axis=-1) - 1.0).max() <= 1e-12
        # world points at several depths along the ray lie on the NDC ray
        worst = 0.0
        on_plane = -(n + o[..., 2:]) / d[..., 2:]                     # the ray parameter at which it crosses the near plane
        for depth in (0.0, 0.5, 2.0, 20.0, 1e3):
            p = R.perspective(o + (on_plane + depth) * d, FOCAL, W, H, n)
            worst = max(worst, np.linalg.norm(np.cross(p - o2, d2), axis=-1).max())
            assert (((p - o2) * d2).sum(-1) >= -1e-12).all() and (p[..., 2] < 1.0).all()       # between the near plane and infinity
        assert worst <= 1e-12, worst
    # the poses of the GPU tests (same seed): no division by a small d_z, values of O(1) -- what their absolute bounds are worked out for
    o2, d2, L = R.ndc_rays(o, d, FOCAL, W, H, 1.0)
    assert np.abs(d[..., 2]).min() >= 0.5 and L.min() >= 2.0 and L.max() <= 3.5 and np.abs(o2).max() <= 5.0


def test_the_sample_references():
    u = np.random.default_rng(0).random((5, 8))
    t = R.disparity_samples(8, 2.0, 6.0, u)
    assert (np.diff(t, axis=-1) > 0).all() and t.min() >= 2.0 and t.max() <= 6.0
    mid = R.disparity_samples(8, 2.0, 6.0, np.full((1, 8), 0.5))
    assert abs(mid[0, 0] - 2.0) <= 1e-12 and abs(mid[0, -1] - 6.0) <= 1e-12
    assert np.allclose(np.diff(1.0 / mid[0]), (1 / 6.0 - 1 / 2.0) / 7, atol=1e-12)       # linear in disparity
    s = R.ndc_samples(8, 0.0, 1.0, u, np.array([2.0, 2.5, 3.0, 3.5, 2.2]))
    assert s.shape == (5, 8) and (s >= 0).all() and (s <= np.array([2.0, 2.5, 3.0, 3.5, 2.2])[:, None]).all()


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root, pb = R.write_llff(str(tmp_path_factory.mktemp("llff") / "scene"), V=10, H=H, W=W, focal=FOCAL, seed=3, factors=(1, 2))
    return root, pb


def test_the_loader_normalises_the_poses(scene):
    root, pb = scene
    ld = LLFFDatasetLoader(root)
    train, val, test = ld.load_dataset(1, W, H, 0.0, 1.0, 8)
    raw = pb[:, :15].reshape(-1, 3, 5)
    # the axis conversion, on a loader that neither scales nor recentres
    plain = LLFFDatasetLoader(root, bd_factor=None, recenter=False)
    plain.load_dataset(1, W, H, 0.0, 1.0, 8)
    assert np.abs(plain.poses[:, :3, 0] - raw[:, :, 1]).max() == 0 and np.abs(plain.poses[:, :3, 1] + raw[:, :, 0]).max() == 0
    assert np.abs(plain.poses[:, :3, 2] - raw[:, :, 2]).max() == 0 and np.abs(plain.poses[:, :3, 3] - raw[:, :, 3]).max() == 0
    assert np.abs(np.linalg.det(plain.poses[:, :3, :3]) - 1.0).max() <= 1e-6            # right-handed after the conversion (the stored rotations are float32)
    assert np.abs(plain.poses[:, 3] - [0, 0, 0, 1]).max() == 0
    # scaling, recentring
    assert abs(ld.bounds.min() * 0.75 - 1.0) <= 1e-6
    assert np.abs(poses_avg(ld.poses) - np.eye(4)).max() <= 1e-6
    want_poses, want_bounds = R.normalised_poses(pb)
    assert np.abs(ld.poses - want_poses).max() <= 1e-9 and np.abs(ld.bounds - want_bounds).max() <= 1e-12
    assert np.abs(recenter_poses(plain.poses) - R.normalised_poses(pb, bd_factor=1.0 / pb[:, 15:].min())[0]).max() <= 1e-9
    assert ld.focal == FOCAL and ld.hwf == (H, W, FOCAL)
    # the hold-out split
    names = lambda ds: [os.path.basename(p) for p in ds.image_paths]
    assert names(val) == names(test) == ["view_000.png", "view_008.png"]
    assert names(train) == [f"view_{i:03d}.png" for i in range(10) if i not in (0, 8)]
    for ds, idx in ((train, [i for i in range(10) if i % 8]), (val, [0, 8])):
        assert np.array_equal(np.stack(ds.camera_params), ld.poses[idx].astype(np.float32))
    assert [len(train), len(val), len(test)] == [8, 2, 2]
    # images come out as rows x cols = H x W, whatever the reference's swapped default would do
    img = train.image_loader(train.image_paths[0])
    assert img.shape == (H, W, 4) and img.dtype == np.float32 and train.image_loader.output_size == (H, W)
    assert (img[..., 3] == 1).all() and 0 <= img.min() and img.max() <= 1
    rb = train.ray_batches(240)
    assert rb.n_pixels == 8 * H * W and len(rb) == 8


def test_the_loader_picks_the_reduced_images(scene):
    root, _ = scene
    ld = LLFFDatasetLoader(root, factor=2)
    train = ld.load_dataset(1, W // 2, H // 2, 0.0, 1.0, 8)[0]
    assert all(os.path.basename(os.path.dirname(p)) == "images_2" for p in train.image_paths)
    assert ld.focal == FOCAL / 2 and ld.hwf == (H // 2, W // 2, FOCAL / 2)
    assert train.image_loader(train.image_paths[0]).shape == (H // 2, W // 2, 4)
    # resized on loading: the focal length follows the width
    ld.load_dataset(1, W, H, 0.0, 1.0, 8)
    assert ld.focal == FOCAL
    with pytest.raises(ValueError, match="images_4"):
        LLFFDatasetLoader(root, factor=4).load_dataset(1, W // 4, H // 4, 0.0, 1.0, 8)


def test_the_loader_refuses_what_does_not_fit(scene, tmp_path):
    root, pb = scene
    with pytest.raises(ValueError, match="aspect"):
        LLFFDatasetLoader(root).load_dataset(1, H, W, 0.0, 1.0, 8)          # width and height swapped
    with pytest.raises(ValueError, match="aspect"):
        LLFFDatasetLoader(root).load_dataset(1, W, H + 2, 0.0, 1.0, 8)
    LLFFDatasetLoader(root).load_dataset(1, 2 * W, 2 * H + 1, 0.0, 1.0, 8)  # within one pixel
    other, _ = R.write_llff(str(tmp_path / "short"), V=10, H=H, W=W, focal=FOCAL, seed=3)
    os.remove(os.path.join(other, "images", "view_004.png"))
    with pytest.raises(ValueError, match="10 views .* 9 images"):
        LLFFDatasetLoader(other).load_dataset(1, W, H, 0.0, 1.0, 8)
    with pytest.raises(ValueError):
        LLFFDatasetLoader(root, ndc=True, spacing="disparity")
    with pytest.raises(ValueError):
        LLFFDatasetLoader(root, spacing="log")


def test_jpeg_photographs_load(tmp_path):
    root, _ = R.write_llff(str(tmp_path / "jpg"), V=3, H=H, W=W, focal=FOCAL, seed=5, suffix=".jpg")
    train = LLFFDatasetLoader(root, holdout=2).load_dataset(1, W, H, 0.0, 1.0, 8)[0]
    assert [os.path.basename(p) for p in train.image_paths] == ["view_001.jpg"]
    assert train.image_loader(train.image_paths[0]).shape == (H, W, 4)


def test_image_loader_keeps_the_swapped_size_by_default(tmp_path):
    from PIL import Image
    from keras_nerf_amd.data.image import ImageLoader
    p = str(tmp_path / "a.png")
    Image.fromarray(np.zeros((30, 40, 3), np.uint8), "RGB").save(p)
    assert ImageLoader(20, 12).output_size == (20, 12) and ImageLoader(20, 12)(p).shape == (20, 12, 4)
    assert ImageLoader(20, 12, height_first=True).output_size == (12, 20) and ImageLoader(20, 12, height_first=True)(p).shape == (12, 20, 4)


def test_the_spiral_path(scene):
    root, _ = scene
    ld = LLFFDatasetLoader(root)
    ld.load_dataset(1, W, H, 0.0, 1.0, 8)
    for n_views, dt in ((120, 0.75), (7, 0.3)):
        path = render_path_spiral(ld.poses, ld.bounds, n_views=n_views, path_dt=dt)
        assert path.shape == (n_views, 4, 4) and path.dtype == np.float32
        Rm = path[:, :3, :3].astype(np.float64)
        assert np.abs(np.swapaxes(Rm, 1, 2) @ Rm - np.eye(3)).max() <= 1e-5
        assert np.abs(np.linalg.det(Rm) - 1.0).max() <= 1e-5
        assert np.abs(path[:, 3] - [0, 0, 0, 1]).max() == 0
        focus = 1.0 / ((1 - dt) / (0.9 * ld.bounds.min()) + dt / (5 * ld.bounds.max()))
        target = (poses_avg(ld.poses) @ [0, 0, -focus, 1])[:3]
        to_focus = target - path[:, :3, 3]
        cos = (-(Rm[:, :, 2]) * to_focus).sum(-1) / np.linalg.norm(to_focus, axis=-1)
        assert cos.min() >= 1 - 1e-5, cos.min()
        rads = np.percentile(np.abs(ld.poses[:, :3, 3]), 90, axis=0)
        assert (np.abs(path[:, :3, 3]) <= rads + 1e-5).all()            # (the average pose is the identity here)
        assert len(np.unique(np.round(path[:, :3, 3], 6), axis=0)) > n_views // 2


def test_rays_generator_checks_its_arguments_without_a_gpu():
    from keras_nerf_amd.data.rays import RaysGenerator
    kw = dict(focal_length=FOCAL, image_width=W, image_height=H, n_sample=8)
    with pytest.raises(ValueError, match="spacing"):
        RaysGenerator(near=2.0, far=6.0, spacing="log", **kw)
    with pytest.raises(ValueError, match="disparity"):
        RaysGenerator(near=0.0, far=1.0, ndc=True, spacing="disparity", **kw)
    for near in (0.0, -1.0):
        with pytest.raises(ValueError, match="near > 0"):
            RaysGenerator(near=near, far=6.0, spacing="disparity", **kw)
    with pytest.raises(ValueError, match="ndc_near"):
        RaysGenerator(near=0.0, far=1.0, ndc=True, ndc_near=0.0, **kw)
    with pytest.raises(ValueError, match="fractions"):
        RaysGenerator(near=2.0, far=6.0, ndc=True, **kw)


def test_the_library_refuses_bad_ray_models_before_any_launch():
    """knerf_generate_rays_ext / knerf_draw_ray_batch_ext return KNERF_ERR_INVALID from their argument checks (no device is touched:
    this runs without a GPU; the pointers are never dereferenced)"""
    import ctypes as C
    from keras_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)
    M = _lib.KnerfRayModel
    gen = lambda near, far, m: lib.knerf_generate_rays_ext(None, None, p, None, 0, 0, 1, H, W, 8, FOCAL, near, far, p, p, p,
                                                           None if m is None else C.byref(m))
    draw = lambda near, far, m: lib.knerf_draw_ray_batch_ext(None, None, p, p, 1, H, W, 3, FOCAL, near, far, 8, 0, 0, 0, 16, None, 0,
                                                             p, p, p, p, None, C.byref(m))
    for fn in (gen, draw):
        for near, far, m in ((0.0, 1.0, M(1, 0, 0.0)), (0.0, 1.0, M(1, 0, -1.0)), (0.0, 1.0, M(1, 0, float("nan"))),
                             (0.0, 6.0, M(0, 1, 1.0)), (-1.0, 6.0, M(0, 1, 1.0)), (0.0, 1.0, M(1, 1, 1.0)), (0.5, 1.0, M(1, 1, 1.0)),
                             (0.0, 1.5, M(1, 0, 1.0)), (-0.1, 1.0, M(1, 0, 1.0)), (2.0, 6.0, M(1, 0, 1.0)),
                             (2.0, 6.0, M(0, 2, 1.0)), (2.0, 6.0, M(2, 0, 1.0))):
            assert fn(near, far, m) == _lib.KNERF_ERR_INVALID, (near, far, m.ndc, m.spacing, m.ndc_near)
            assert lib.knerf_last_error(None)
    assert lib.knerf_generate_rays_ext(None, None, None, None, 0, 0, 1, H, W, 8, FOCAL, 0.0, 1.0, p, p, p, None) == _lib.KNERF_ERR_INVALID
