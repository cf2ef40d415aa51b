"""Training on random ray batches, on the GPU: the kernel of csrc/raybatch.hip against its specification -- the pixels of
`ray_batch_permutation`, the rays of knerf_generate_rays for those pixels, the images' colours, the jitter restated through
oracle.philox4x32, all bit for bit; `RayBatchDataset` epochs; `NeRF.train_step` / `fit` on ray batches; and a small convergence
comparison with image-mode training."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
NEAR, FAR = 2.0, 6.0


def _poses(V):
    from keras_nerf_amd.data.utils import pose_spherical      # the cameras of tests/procedural_scene.make_scene
    return np.stack([pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]).astype(np.float32)


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def ctx():
    from keras_nerf_amd.runtime import KnerfContext
    c = KnerfContext(white_background=True)
    yield c
    c.close()


@pytest.mark.parametrize("V,H,W,C,N", [(7, 24, 24, 3, 64), (7, 24, 24, 4, 64), (100, 128, 128, 4, 16), (100, 128, 128, 3, 16)])
def test_the_kernel_draws_what_the_specification_says(ctx, V, H, W, C, N):
    from keras_nerf_amd.data import ray_batch_permutation
    P, focal = V * H * W, 1.2 * W
    g = torch.Generator(device="cuda").manual_seed(V + C)
    images = torch.rand((V, H, W, C), device="cuda", generator=g)
    c2w = torch.as_tensor(_poses(V), device="cuda")
    ro, rd, _ = ctx.generate_rays(c2w, focal, H, W, NEAR, FAR, N, None, seed=1)
    n = min(32768, P - 1000) // 64 * 64
    for seed, epoch, first in ((0, 0, 0), (5, 3, 1000), (2 ** 40 + 9, 2 ** 33 + 1, P - n)):
        # injected noise
        noise = torch.rand((n, N), device="cuda", generator=g)
        o, d, t, target, index = ctx.draw_ray_batch(images, c2w, focal, NEAR, FAR, N, seed, epoch, first, n, noise=noise, want_index=True)
        want = ray_batch_permutation(P, seed, epoch, np.arange(first, first + n))
        assert index.dtype == torch.int64 and np.array_equal(index.cpu().numpy(), want), (seed, epoch, first)
        assert len(np.unique(want)) == n
        assert torch.equal(_bits(o), _bits(ro.reshape(P, 3)[index])) and torch.equal(_bits(d), _bits(rd.reshape(P, 3)[index]))
        assert torch.equal(_bits(target), _bits(images.reshape(P, C)[index, :3]))
        full = torch.zeros((P, N), device="cuda")
        full[index] = noise
        rt = ctx.generate_rays(c2w, focal, H, W, NEAR, FAR, N, full.reshape(V, H, W, N))[2]
        assert torch.equal(_bits(t), _bits(rt.reshape(P, N)[index]))
        # Philox: counter (n >> 2, slot, noise_stream, 2) under the key `seed`
        stream = 77 + epoch % 5
        o2, d2, t2, target2 = ctx.draw_ray_batch(images, c2w, focal, NEAR, FAR, N, seed, epoch, first, n, noise_stream=stream)
        assert torch.equal(_bits(o2), _bits(o)) and torch.equal(_bits(d2), _bits(d)) and torch.equal(_bits(target2), _bits(target))
        s, k = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(N, dtype=np.uint32), indexing="ij")
        counter = np.stack([k >> 2, s, np.full_like(s, stream), np.full_like(s, 2)], -1)
        key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32), (n, N, 2))
        words = O.philox4x32(counter, key)
        u = (np.take_along_axis(words, (k & 3)[..., None].astype(np.int64), -1)[..., 0] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        f = np.float32
        step = (f(FAR) - f(NEAR)) / f(N - 1)
        base = f(NEAR) + k.astype(f) * step
        base[:, -1] = f(FAR)
        interval = (f(FAR) - f(NEAR)) / f(N)
        tv = np.clip((base + u * interval) - interval / f(2), f(NEAR), f(FAR)).astype(f)
        assert np.array_equal(t2.cpu().numpy().view(np.int32), tv.view(np.int32)), (seed, epoch, first)
        assert not torch.equal(t2, ctx.draw_ray_batch(images, c2w, focal, NEAR, FAR, N, seed, epoch, first, n, noise_stream=stream + 1)[2])
    with pytest.raises(ValueError):
        ctx.draw_ray_batch(images, c2w, focal, NEAR, FAR, N, 0, 0, P - n + 1, n)
    with pytest.raises(ValueError):
        ctx.draw_ray_batch(images[..., :2], c2w, focal, NEAR, FAR, N, 0, 0, 0, n)


def _loaded(tmp_path, n=(6, 2, 3), batch=1):
    from keras_nerf_amd.data.loader import DatasetLoader
    from tests.synthetic_scene import write
    root = write(str(tmp_path / "scene"), n=n)
    return DatasetLoader(root, white_background=True).load_dataset(batch, 24, 24, NEAR, FAR, 64)


def test_an_epoch_of_the_dataset_visits_distinct_pixels(tmp_path):
    from keras_nerf_amd.runtime import draw_ray_batch
    train = _loaded(tmp_path)[0]
    rb = train.ray_batches(1024, seed=4)
    P = 6 * 24 * 24
    assert len(rb) == P // 1024 == 3
    epochs = []
    for _ in range(2):
        idx = []
        for target, (o, d, t) in rb:
            assert target.shape == (1024, 3) and o.shape == d.shape == (1024, 3) and t.shape == (1024, 64) and t.is_cuda
            dev, cams = rb._resident_all()
            perm, first, n = rb.last_draw
            o2, d2, _, target2, index = draw_ray_batch(dev, cams, rb._rg.focal_length, NEAR, FAR, 64, 4, perm, first, n, want_index=True)
            assert torch.equal(target, target2) and torch.equal(o, o2) and torch.equal(d, d2)
            idx.append(index.cpu().numpy())
        idx = np.concatenate(idx)
        assert len(idx) == 3 * 1024 == len(np.unique(idx)) and idx.min() >= 0 and idx.max() < P
        epochs.append(idx)
    assert (epochs[0] == epochs[1]).sum() < 20
    # the image-mode dataset shares the resident copy: its batches are those images
    img, _ = next(iter(train))
    assert img.shape == (1, 24, 24, 4) and (rb._resident_all()[0] == img).flatten(1).all(1).any()


def _nerf(batch=1, wh=24, chunk=192, seed=0, **kw):
    from keras_nerf_amd.model.nerf.nerf import NeRF
    nerf = NeRF(seed=seed)
    nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=batch, image_height=wh, image_width=wh, ray_chunks=chunk, white_background=True, **kw)
    return nerf


def test_a_ray_step_is_train_batch_and_adam_and_nothing_else(tmp_path):
    from keras_nerf_amd.model.nerf.metrics import NAMES
    train = _loaded(tmp_path)[0]
    target, (o, d, t) = next(iter(train.ray_batches(960, seed=1)))
    a, b = _nerf(deterministic=True), _nerf(deterministic=True)
    logs = a.train_step((target, (o, d, t)))
    assert sorted(logs) == ["coarse_loss", "coarse_psnr", "fine_loss", "fine_psnr"] and len(logs) == 4
    loss = torch.zeros(2, device="cuda")
    ci, fi = torch.empty((960, 3), device="cuda"), torch.empty((960, 3), device="cuda")
    b._ctx.train_batch(o, d, t, target, None, b._next_seed(), 192, loss, ci, fi)
    b._ctx.apply_adam()
    for net in (0, 1):
        assert np.array_equal(a._ctx.get_weights(net), b._ctx.get_weights(net))
    want = {"coarse_loss": float(loss[0]), "fine_loss": float(loss[1]), "coarse_psnr": -10 * np.log10(float(loss[0])),
            "fine_psnr": -10 * np.log10(float(loss[1]))}
    for k, v in want.items():
        assert abs(logs[k] - v) <= 1e-5 * max(1.0, abs(v)), (k, logs[k], v)
    with pytest.raises(ValueError, match="ray_chunks"):
        a.train_step((target[:100], (o[:100], d[:100], t[:100])))
    img, rays = next(iter(train))
    logs6 = a.train_step((img, rays))
    assert tuple(logs6) == NAMES and len(dict(logs6)) == 6


def test_fit_on_ray_batches_with_validation_and_the_grid_updater(tmp_path):
    from keras_nerf_amd.model.nerf.callback import OccupancyGridUpdater
    from keras_nerf_amd.model.nerf.metrics import NAMES
    train, val, _ = _loaded(tmp_path)
    nerf = _nerf()
    upd = OccupancyGridUpdater(update_every=2, warmup_steps=2, resolution=32)
    rb = train.ray_batches(576)
    h = nerf.fit(rb, epochs=2, validation_data=val, callbacks=[upd], verbose=0)
    assert sorted(h.history) == sorted(["coarse_loss", "coarse_psnr", "fine_loss", "fine_psnr"] + ["val_" + k for k in NAMES])
    assert all(len(v) == 2 and np.all(np.isfinite(v)) for v in h.history.values())
    assert h.params["steps"] == len(rb) == 6 and upd.updates >= 1
    nerf._ctx.poll_nonfinite(wait=True)


def test_ray_batches_converge_no_worse_than_whole_images(ctx):
    """Held-out fine PSNR after 300 steps of 32,768 rays from the same initial weights: whole images (batch 2) against ray batches.
    0.3 dB is the wander of a single training leg (README parity row): the assertion says "not worse".
    Measured on MI355X, two runs: image mode 27.01 and 26.99 dB, ray mode 31.39 and 30.99 dB."""
    from keras_nerf_amd.data.utils import get_focal_from_fov
    from tests.procedural_scene import FOV, make_scene
    wh, V, n_train, steps, rays = 128, 28, 24, 300, 32768
    o, d, t, img = make_scene(ctx, wh=wh, n_views=V, scale=1.6)
    c2w = torch.as_tensor(_poses(V), device="cuda")
    focal = get_focal_from_fov(FOV, wh)
    assert torch.equal(ctx.generate_rays(c2w, focal, wh, wh, NEAR, FAR, 64, None, seed=2026)[1], d)      # the scene's cameras
    u = torch.rand((2, wh, wh, 128), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))

    def held_out(nerf):
        se = 0.0
        for a in range(n_train, V, 2):
            fine = nerf.predict_and_render_images((o[a:a + 2], d[a:a + 2], t[a:a + 2]), u=u, outputs=("image",))[1]["image"]
            se += float(((fine - img[a:a + 2]) ** 2).sum())
        return -10 * np.log10(se / ((V - n_train) * wh * wh * 3))

    image_mode = _nerf(batch=2, wh=wh, chunk=4096)
    order = np.random.default_rng(5).integers(0, n_train, (steps, 2))
    for s in range(steps):
        idx = torch.as_tensor(order[s], device="cuda")
        oo, dd, tt = ctx.generate_rays(c2w[idx], focal, wh, wh, NEAR, FAR, 64, None, seed=11, stream_id=s)
        image_mode.train_step((img[idx], (oo, dd, tt)), with_metrics=False)
    image_mode._ctx.poll_nonfinite(wait=True)
    ray_mode = _nerf(batch=2, wh=wh, chunk=4096)
    train_img = img[:n_train].contiguous()
    for s in range(steps):
        per_epoch = n_train * wh * wh // rays
        oo, dd, tt, target = ctx.draw_ray_batch(train_img, c2w[:n_train], focal, NEAR, FAR, 64, 11, s // per_epoch, (s % per_epoch) * rays, rays,
                                                noise_stream=s)
        ray_mode.train_step((target, (oo, dd, tt)), with_metrics=False)
    ray_mode._ctx.poll_nonfinite(wait=True)
    ps = {"image": held_out(image_mode), "ray": held_out(ray_mode)}
    print(f"held-out fine PSNR after {steps} steps: image mode {ps['image']:.2f} dB, ray mode {ps['ray']:.2f} dB")
    assert ps["ray"] >= ps["image"] - 0.3, ps
