"""Forward-facing scenes on the GPU: the kernels of csrc/rays_ext.hip against the fp64 restatements of
tests/forward_facing_reference.py and, where the two overlap, against the plain ray kernels bit for bit; then the LLFF loader, `fit`
and a spiral-path render end to end (tests/README_forward_facing.md).

Shapes: V = 3 views of 12 x 20 pixels, focal 18, N = 8 samples; poses with rotations within +-0.35 rad about each axis and
translations within +-0.5, for which |d_z| >= 0.5 and the NDC lengths lie in [2, 3.5] (tests/test_forward_facing_host.py asserts it
for this seed), so no division is ill-conditioned and no case is excluded."""
import numpy as np
import pytest
import torch

from tests import forward_facing_reference as R

pytestmark = pytest.mark.gpu
V, H, W, FOCAL, N = 3, 12, 20, 18.0, 8
P = V * H * W


def _bits(x):
    return x.contiguous().view(torch.int32)


def _model(ndc=0, spacing=0, ndc_near=1.0):
    from keras_nerf_amd import _lib
    return _lib.KnerfRayModel(ndc, spacing, ndc_near)


@pytest.fixture(scope="module")
def ctx():
    from keras_nerf_amd.runtime import KnerfContext
    c = KnerfContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene(ctx):
    """cameras, images, injected noise and the plain kernels' fp32 pinhole rays, shared and left unchanged"""
    g = torch.Generator(device="cuda").manual_seed(5)
    c2w = torch.as_tensor(R.random_poses(V, R.GPU_POSE_SEED), device="cuda")
    noise = torch.rand((V, H, W, N), device="cuda", generator=g)
    images = torch.rand((V, H, W, 4), device="cuda", generator=g)
    o, d, _ = ctx.generate_rays(c2w, FOCAL, H, W, 2.0, 6.0, N, noise)
    return dict(c2w=c2w, noise=noise, images=images, o=o, d=d, o64=o.double().cpu().numpy(), d64=d.double().cpu().numpy(),
                noise64=noise.double().cpu().numpy())


def _err(got, want):
    return float(np.abs(got.double().cpu().numpy() - want).max())


def test_ndc_view_rays_match_the_fp64_reference(ctx, scene):
    """fed the fp32 pinhole rays the plain kernel writes, so that only the new arithmetic is measured.  Bound 1e-5 absolute on values
    of O(1 - 5): the fp32 restatement of the same formulas is within 1e-6 of fp64; a wrong sign, a swapped W / H or a missing shift
    to the near plane is off by orders of magnitude."""
    from keras_nerf_amd.data.rays import RaysGenerator
    want_o, want_d, L = R.ndc_rays(scene["o64"], scene["d64"], FOCAL, W, H, 1.0)
    want_t = R.ndc_samples(N, 0.0, 1.0, scene["noise64"], L)
    o, d, t = ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 0.0, 1.0, N, _model(ndc=1), scene["noise"])
    errs = (_err(o, want_o), _err(d, want_d), _err(t, want_t))
    print("NDC view rays, max |gpu - fp64| of o, d, t:", errs)
    assert max(errs) <= 1e-5, errs
    assert float((d.norm(dim=-1) - 1).abs().max()) <= 1e-6
    # the public class calls the same entry point
    o2, d2, t2 = RaysGenerator(FOCAL, W, H, 0.0, 1.0, N, ndc=True, ndc_near=1.0)(scene["c2w"], noise=scene["noise"])
    assert torch.equal(_bits(o2), _bits(o)) and torch.equal(_bits(d2), _bits(d)) and torch.equal(_bits(t2), _bits(t))
    o1, d1, t1 = RaysGenerator(FOCAL, W, H, 0.0, 1.0, N, ndc=True)(scene["c2w"][1], noise=scene["noise"][1])
    assert o1.shape == (H, W, 3) and torch.equal(_bits(o1), _bits(o[1])) and torch.equal(_bits(t1), _bits(t[1]))
    # another near plane: the same bound
    oh, dh, th = ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 0.0, 1.0, N, _model(ndc=1, ndc_near=0.5), scene["noise"])
    wo, wd, Lh = R.ndc_rays(scene["o64"], scene["d64"], FOCAL, W, H, 0.5)
    assert max(_err(oh, wo), _err(dh, wd), _err(th, R.ndc_samples(N, 0.0, 1.0, scene["noise64"], Lh))) <= 1e-5


def test_an_ndc_ray_batch_holds_the_view_rays_bit_for_bit(ctx, scene):
    m = _model(ndc=1)
    vo, vd, _ = ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 0.0, 1.0, N, m, scene["noise"])
    g = torch.Generator(device="cuda").manual_seed(6)
    for seed, epoch, first, n in ((0, 0, 0, P), (5, 3, 17, 700), (2 ** 40 + 9, 2 ** 33 + 1, P - 300, 300)):
        noise = torch.rand((n, N), device="cuda", generator=g)
        o, d, t, target, index = ctx.draw_ray_batch(scene["images"], scene["c2w"], FOCAL, 0.0, 1.0, N, seed, epoch, first, n, noise=noise,
                                                    want_index=True, ray_model=m)
        assert len(torch.unique(index)) == n and int(index.min()) >= 0 and int(index.max()) < P
        assert torch.equal(_bits(o), _bits(vo.reshape(P, 3)[index])) and torch.equal(_bits(d), _bits(vd.reshape(P, 3)[index]))
        assert torch.equal(_bits(target), _bits(scene["images"].reshape(P, 4)[index, :3]))
        full = torch.zeros((P, N), device="cuda")
        full[index] = noise
        vt = ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 0.0, 1.0, N, m, full.reshape(V, H, W, N))[2]
        assert torch.equal(_bits(t), _bits(vt.reshape(P, N)[index]))
        # the same pixels as a plain batch draws at these positions
        assert torch.equal(index, ctx.draw_ray_batch(scene["images"], scene["c2w"], FOCAL, 2.0, 6.0, N, seed, epoch, first, n, want_index=True)[4])


def test_pinhole_rays_with_linear_spacing_are_the_plain_kernels_bits(ctx, scene):
    m = _model()
    c2w, images = scene["c2w"], scene["images"]
    for kw in (dict(noise=scene["noise"]), dict(noise=None, seed=77, stream_id=3), dict(noise=None, seed=2 ** 40 + 1, stream_id=2 ** 33)):
        plain = ctx.generate_rays(c2w, FOCAL, H, W, 2.0, 6.0, N, **kw)
        ext = ctx.generate_rays_ext(c2w, FOCAL, H, W, 2.0, 6.0, N, m, **kw)
        for a, b, name in zip(plain, ext, "odt"):
            assert torch.equal(_bits(a), _bits(b)), (name, kw.get("seed"))
    n, first = 704, 9
    for kw in (dict(noise=torch.rand((n, N), device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))),
               dict(noise_stream=0), dict(noise_stream=2 ** 33 + 5)):
        for seed, epoch in ((0, 0), (2 ** 40 + 9, 4)):
            plain = ctx.draw_ray_batch(images, c2w, FOCAL, 2.0, 6.0, N, seed, epoch, first, n, want_index=True, **kw)
            ext = ctx.draw_ray_batch(images, c2w, FOCAL, 2.0, 6.0, N, seed, epoch, first, n, want_index=True, ray_model=m, **kw)
            for a, b, name in zip(plain, ext, ("o", "d", "t", "target", "index")):
                assert torch.equal(a, b) and (a.dtype != torch.float32 or torch.equal(_bits(a), _bits(b))), (name, seed, epoch)
    # three channels, no index
    rgb = images[..., :3].contiguous()
    plain = ctx.draw_ray_batch(rgb, c2w, FOCAL, 2.0, 6.0, N, 1, 0, 0, 64, noise_stream=1)
    ext = ctx.draw_ray_batch(rgb, c2w, FOCAL, 2.0, 6.0, N, 1, 0, 0, 64, noise_stream=1, ray_model=m)
    assert len(ext) == 4 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(plain, ext))


def test_disparity_spacing_matches_the_fp64_reference(ctx, scene):
    """near 2, far 6: bound 2e-6 absolute on values up to 6 (four fp32 roundings of quantities <= 0.5 and one reciprocal; the fp32
    restatement of the formula is within 2.4e-7 of fp64)"""
    near, far, m = 2.0, 6.0, _model(spacing=1)
    o, d, t = ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, near, far, N, m, scene["noise"])
    assert torch.equal(_bits(o), _bits(scene["o"])) and torch.equal(_bits(d), _bits(scene["d"]))        # the rays stay pinhole rays
    err = _err(t, R.disparity_samples(N, near, far, scene["noise64"]))
    print("disparity spacing, max |gpu - fp64| of t:", err)
    assert err <= 2e-6, err
    assert bool((t[..., 1:] > t[..., :-1]).all())
    half = ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, near, far, N, m, torch.full((V, H, W, N), 0.5, device="cuda"))[2]
    assert float((half[..., 0] - near).abs().max()) <= 2e-6 and float((half[..., -1] - far).abs().max()) <= 2e-6
    assert _err(half, R.disparity_samples(N, near, far, np.full((V, H, W, N), 0.5))) <= 2e-6
    # a ray batch carries the same positions for the same noise
    n = P
    noise = scene["noise"].reshape(P, N)
    _, _, bt, _, index = ctx.draw_ray_batch(scene["images"], scene["c2w"], FOCAL, near, far, N, 3, 1, 0, n, noise=noise, want_index=True, ray_model=m)
    full = torch.zeros((P, N), device="cuda")
    full[index] = noise
    vt = ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, near, far, N, m, full.reshape(V, H, W, N))[2]
    assert torch.equal(_bits(bt), _bits(vt.reshape(P, N)[index]))
    with pytest.raises(Exception):
        ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 0.0, far, N, m, scene["noise"])
    with pytest.raises(Exception):
        ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 0.0, 1.0, N, _model(ndc=1, spacing=1), scene["noise"])


def test_ndc_samples_from_the_philox_stream(ctx, scene):
    from keras_nerf_amd.data.rays import RaysGenerator
    L = torch.as_tensor(R.ndc_rays(scene["o64"], scene["d64"], FOCAL, W, H, 1.0)[2], device="cuda")
    a, b = (RaysGenerator(FOCAL, W, H, 0.0, 1.0, N, seed=21, ndc=True) for _ in range(2))
    oa, da, ta = a(scene["c2w"])
    ob, db, tb = b(scene["c2w"])
    assert torch.equal(_bits(ta), _bits(tb)) and torch.equal(_bits(oa), _bits(ob)) and torch.equal(_bits(da), _bits(db))
    ta2 = a(scene["c2w"])[2]
    assert not torch.equal(ta, ta2) and torch.equal(_bits(ta2), _bits(b(scene["c2w"])[2]))       # the next call: new jitter, again shared
    assert not torch.equal(ta, RaysGenerator(FOCAL, W, H, 0.0, 1.0, N, seed=22, ndc=True)(scene["c2w"])[2])
    for t in (ta, ta2):
        assert bool((t >= 0).all()) and bool((t.double() <= (L * (1 + 1e-6))[..., None]).all())
        assert bool((t[..., 1:] >= t[..., :-1]).all())
        assert float((t[..., -1].double() / L).min()) > 0.9 and float((t[..., 0].double() / L).max()) < 0.1     # the whole ray is covered
    # the entry point with explicit counters: (seed, stream) names the jitter
    m = _model(ndc=1)
    t1 = ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 0.0, 1.0, N, m, seed=21, stream_id=1)[2]
    assert torch.equal(_bits(t1), _bits(ta)) and torch.equal(_bits(ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 0.0, 1.0, N, m, seed=21, stream_id=2)[2]), _bits(ta2))
    # a sub-range of the ray
    tq = ctx.generate_rays_ext(scene["c2w"], FOCAL, H, W, 0.25, 0.75, N, m, seed=21, stream_id=1)[2].double()
    assert bool((tq >= 0.25 * L[..., None] * (1 - 1e-6)).all()) and bool((tq <= 0.75 * L[..., None] * (1 + 1e-6)).all())


def test_llff_directory_to_fit_to_spiral_render(tmp_path):
    """the data layer, both training modes and a render on 12 x 20 images; no assertion that the loss falls (convergence evidence
    belongs to tools/forward_facing_bench.py, not to a test that could flake)"""
    from keras_nerf_amd.data.llff import LLFFDatasetLoader
    from keras_nerf_amd.data.rays import RaysGenerator
    from keras_nerf_amd.data.utils import render_path_spiral
    from keras_nerf_amd.model.nerf.metrics import NAMES
    from keras_nerf_amd.model.nerf.nerf import NeRF
    root, _ = R.write_llff(str(tmp_path / "scene"), V=10, H=H, W=W, focal=FOCAL, seed=3)
    ld = LLFFDatasetLoader(root)
    n_coarse = 32
    train, val, test = ld.load_dataset(1, W, H, 0.0, 1.0, n_coarse)
    nerf = NeRF(n_coarse=n_coarse, n_fine=32, n_layers=4, dense_units=64, skip_layer=2, seed=1)
    nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=1, image_height=H, image_width=W, ray_chunks=240)
    before = [nerf.coarse.get_flat_weights().copy(), nerf.fine.get_flat_weights().copy()]
    img, (o, d, t) = next(iter(train))
    assert img.shape == (1, H, W, 4) and o.shape == d.shape == (1, H, W, 3) and t.shape == (1, H, W, n_coarse)
    assert float((o[..., 2] + 1).abs().max()) <= 1e-5 and float((d.norm(dim=-1) - 1).abs().max()) <= 1e-5       # NDC rays
    h = nerf.fit(train, epochs=1, validation_data=val, verbose=0)
    assert h.params["steps"] == 8 and sorted(h.history) == sorted(list(NAMES) + ["val_" + k for k in NAMES])
    assert all(len(v) == 1 and np.all(np.isfinite(v)) for v in h.history.values()), h.history
    mid = [nerf.coarse.get_flat_weights().copy(), nerf.fine.get_flat_weights().copy()]
    assert all(not np.array_equal(a, b) for a, b in zip(before, mid))
    rb = train.ray_batches(240, seed=2, steps_per_epoch=3)
    target, (ro, rd, rt) = next(iter(rb))
    assert target.shape == ro.shape == rd.shape == (240, 3) and rt.shape == (240, n_coarse)
    assert float((ro[..., 2] + 1).abs().max()) <= 1e-5                                                             # the model is passed through
    h = nerf.fit(rb, epochs=1, verbose=0)
    assert h.params["steps"] == 3 and all(np.all(np.isfinite(v)) for v in h.history.values()), h.history
    assert all(not np.array_equal(a, b) for a, b in zip(mid, [nerf.coarse.get_flat_weights(), nerf.fine.get_flat_weights()]))
    logs = nerf.test_step(next(iter(test)))
    assert tuple(logs) == NAMES and all(np.isfinite(float(logs[k])) for k in NAMES), dict(logs)
    path = render_path_spiral(ld.poses, ld.bounds, n_views=8)
    rg = RaysGenerator(ld.focal, W, H, 0.0, 1.0, n_coarse, ndc=True)
    image = nerf.predict_and_render_images(rg(path[3:4]), outputs=("image",))[1]["image"]
    assert image.shape == (1, H, W, 3) and bool(torch.isfinite(image).all()) and float(image.min()) >= 0 and float(image.max()) <= 1
    nerf._ctx.poll_nonfinite(wait=True)
