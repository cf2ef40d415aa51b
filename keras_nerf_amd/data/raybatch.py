"""Training on rays drawn at random over all pixels of all images of a dataset (csrc/raybatch.hip).

`ray_batch_permutation` restates the kernel's pixel permutation in NumPy -- it is the specification the kernel is tested against.
`RayBatchDataset` (from `RayImageDataset.ray_batches`) yields one batch of rays per train step, drawn by ONE kernel launch from the
dataset's device-resident images and camera matrices: the host passes a position, builds no index tensor and waits for nothing."""
from __future__ import annotations

import numpy as np

PERM_ROUNDS = 6
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key: int):
    """one Philox-4x32-10 block: counter = four 32-bit words, key = 64 bits -> four 32-bit words (Python integers)"""
    c = [int(x) & _M32 for x in counter]
    k0, k1 = key & _M32, (key >> 32) & _M32
    for _ in range(10):
        p0, p1 = c[0] * 0xD2511F53, c[2] * 0xCD9E8D57
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & _M32, (p0 >> 32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c


def permutation_keys(seed: int, epoch: int):
    """the six round keys: two Philox blocks with counter (j, epoch lo, epoch hi, 3) under the key `seed`"""
    seed, epoch = int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1)
    words = [w for j in range(2) for w in philox4x32_10((j, epoch & _M32, epoch >> 32, 3), seed)]
    return words[:PERM_ROUNDS]


def _fmix32(h):
    """the murmur3 finaliser on uint32 arrays"""
    h = h ^ (h >> np.uint32(16)); h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13)); h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def ray_batch_permutation(P: int, seed: int, epoch: int, positions, return_walk: bool = False):
    """perm(seed, epoch)(positions): the pixel of the dataset (flat index below P = views x height x width) at each position of an
    epoch.  A keyed bijection of [0, P) evaluated per position: a six-round Feistel network over b = bit_length(P - 1) bits -- a high
    half of b // 2 bits and a low half of b - b // 2 bits that swap places every round, round function the murmur3 finaliser of
    (half ^ round key) -- applied again while the value is not below P (cycle walking; the domain 2^b is below 2 P, so walks are
    short, and they end because they follow a cycle of a permutation that starts inside [0, P)).
    return_walk: also the number of network applications each position took (1 = no walk)."""
    P = int(P)
    if not 0 < P < 2 ** 40:
        raise ValueError(f"a dataset of {P} pixels: the permutation covers 1 <= P < 2^40")
    pos = np.atleast_1d(np.asarray(positions)).astype(np.uint64)
    if pos.size and int(pos.max()) >= P:
        raise ValueError(f"positions must lie in [0, {P})")
    b = (P - 1).bit_length()
    hi, lo = b // 2, b - b // 2
    keys = [np.uint32(k) for k in permutation_keys(seed, epoch)]
    out = pos.copy()
    walk = np.zeros(pos.shape, np.int32)
    todo = np.arange(pos.size)
    x = pos
    with np.errstate(over="ignore"):
        while todo.size:
            L, R = (x >> np.uint64(lo)).astype(np.uint32), (x & np.uint64((1 << lo) - 1)).astype(np.uint32)
            wl = hi
            for k in keys:
                L, R = R, (L ^ _fmix32(R ^ k)) & np.uint32((1 << wl) - 1)
                wl = b - wl
            x = (L.astype(np.uint64) << np.uint64(lo)) | R.astype(np.uint64)
            out[todo] = x
            walk[todo] += 1
            again = x >= np.uint64(P)
            todo, x = todo[again], x[again]
    out = out.astype(np.int64)
    return (out, walk) if return_walk else out


def rank_positions(step: int, rays_per_step: int, rank: int = 0, world: int = 1):
    """(first, count): the positions of a permutation that rank `rank` of `world` draws in step `step` -- its 1/world slice of the
    step's `rays_per_step` (the global count) consecutive positions, so the ranks' slices are disjoint and together are exactly
    what a single process draws"""
    if rays_per_step % world:
        raise ValueError(f"rays_per_step = {rays_per_step} (the global count) is not divisible by {world} replicas")
    n = rays_per_step // world
    return step * rays_per_step + rank * n, n


def loader_output_size(image_loader):
    """(rows, cols) of the images a loader returns: its `output_size`, or the reference's swapped (image_width, image_height) for a
    loader that does not say (ImageLoader's default)"""
    size = getattr(image_loader, "output_size", None)
    return tuple(int(v) for v in size) if size is not None else (int(image_loader.image_width), int(image_loader.image_height))


class RayBatchDataset:
    """Re-iterable; one iteration is one epoch of `len(self)` steps, each yielding (target [n,3], (o [n,3], d [n,3], t [n,n_coarse]))
    on the device, n = rays_per_step / world.

    Without `steps_per_epoch` an epoch is one permutation of the P pixels: P // rays_per_step steps, the tail of fewer than
    rays_per_step pixels dropped (the next epoch is another permutation, so no pixel is starved).  With it, epochs of that many
    steps continue through the permutation and start the next one when fewer than rays_per_step positions are left.

    alpha=True: the target is [n,4], the images' alpha behind the colour (gathered from the resident images by the flat pixel index the
    draw returns), for the grid optimisers' RGBA training; o, d, t and the colour are what they are without it.

    set_depth(depth, weight): per-pixel depth targets for the grid optimisers' depth_loss= keyword; every batch then leaves the drawn
    rays' targets and weights in `last_depth`, gathered by the same flat pixel index."""

    def __init__(self, images, rays_per_step: int, seed: int = 0, steps_per_epoch: int = None, alpha: bool = False):
        self.alpha = bool(alpha)
        self._images = images                                  # the RayImageDataset whose pixels are drawn
        self.rays_per_step, self.seed = int(rays_per_step), int(seed)
        self.steps_per_epoch = None if steps_per_epoch is None else int(steps_per_epoch)
        ld = images.image_loader
        self.n_views = len(images.image_paths)
        self._rows, self._cols = loader_output_size(ld)
        self.n_pixels = self.n_views * self._rows * self._cols
        if self.rays_per_step <= 0 or self.rays_per_step > self.n_pixels:
            raise ValueError(f"rays_per_step = {rays_per_step}: the dataset has {self.n_pixels} pixels")
        if self.steps_per_epoch is not None and self.steps_per_epoch <= 0:
            raise ValueError("steps_per_epoch must be positive")
        self._perm, self._step, self._drawn = 0, 0, 0          # permutation in use, steps taken from it, batches drawn in all
        self._rg, self.last_draw = None, None
        self._cameras, self.last_view = None, None             # set_cameras: who says where the cameras stand; the rays' views
        self._depth, self.last_depth = None, None              # set_depth: the depth maps (and weights); the rays' (z, c)

    def set_cameras(self, provider):
        """provider: None (default: the dataset's own camera matrices, and the batches are what they always were) or a callable
        returning the [V,4,4] float32 device tensor of camera-to-world matrices to draw the NEXT batch with, asked once per batch
        (baked_pose.PoseOptimizer.poses while the poses are refined).  With a provider every draw also leaves the camera of each ray
        in `last_view` (int32 [n] on the device): the flat pixel index of knerf_draw_ray_batch over the pixels per view."""
        if provider is not None and not callable(provider):
            raise ValueError(f"cameras must be None or a callable returning a [V,4,4] device tensor, got {provider!r}")
        self._cameras = provider
        if provider is None:
            self.last_view = None

    def set_depth(self, depth, weight=None):
        """depth: None (default: no flat index is requested, last_depth is None and the batches are what they always were) or a
        [V,H,W] float32 map of depth targets at the dataset's image size, in ray-parameter units (data/depth.py converts z-depth,
        distances and structure-from-motion points); weight: None or a [V,H,W] float32 map of weights >= 0 (0: the pixel has no
        target).  Arrays or tensors; they are kept on the device and count against the dataset's device_cache_gb beside the images.
        Every draw then leaves last_depth = (z [n], c [n] | None), the maps at the drawn rays' pixels (GridOptimizer.fit reads it)."""
        if depth is None:
            if weight is not None:
                raise ValueError("a depth weight without depth")
            self._depth, self.last_depth = None, None
            return
        want = (self.n_views, self._rows, self._cols)
        maps = []
        for name, m in (("depth", depth), ("weight", weight)):
            if m is None:
                maps.append(None)
                continue
            if tuple(m.shape) != want:
                raise ValueError(f"{name} must be {list(want)} (views, rows, columns of the dataset's images), got {list(m.shape)}")
            maps.append(m)
        need = self.n_pixels * 4 * (4 + sum(m is not None for m in maps))
        if need > self._images.device_cache_gb * 1e9:
            raise ValueError(f"depth maps beside the images need {need / 1e9:.2f} GB on the device: more than device_cache_gb = "
                             f"{self._images.device_cache_gb}")
        import torch
        to_dev = lambda m: None if m is None else (m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m, np.float32))).to(
            "cuda", torch.float32).contiguous()
        self._depth = (to_dev(maps[0]), to_dev(maps[1]))

    def ray_model(self):
        """the struct knerf_ray_model the batches are drawn with, None for the plain pinhole rays (the ray generator's own answer)"""
        if self._rg is None:
            self._rg = self._images._rg_factory(self._images._placement()[0])
        return getattr(self._rg, "ray_model", None)

    def __len__(self):
        return self.steps_per_epoch if self.steps_per_epoch is not None else self.n_pixels // self.rays_per_step

    def schedule(self):
        """[(permutation, step within it)] of the next iteration's steps; advances the dataset's position"""
        per_perm = self.n_pixels // self.rays_per_step
        out = []
        if self.steps_per_epoch is None:
            out = [(self._perm, s) for s in range(per_perm)]
            self._perm += 1
        else:
            for _ in range(self.steps_per_epoch):
                if self._step >= per_perm:
                    self._perm, self._step = self._perm + 1, 0
                out.append((self._perm, self._step))
                self._step += 1
        return out

    def _resident_all(self):
        """(images [V,H,W,4], cams [V,4,4]) on the device, every image decoded and uploaded (the cache of the image-mode dataset)"""
        ds = self._images
        need = self.n_pixels * 4 * 4
        if need > ds.device_cache_gb * 1e9:
            raise ValueError(f"ray batches need the whole dataset on the device: {need / 1e9:.2f} GB of images exceed "
                             f"device_cache_gb = {ds.device_cache_gb}")
        dev, have, cams = ds._resident((self._rows, self._cols, 4))      # (rows, cols) as the image loader resizes
        missing = [i for i in range(self.n_views) if not have[i]]
        for k in range(0, len(missing), 16):                   # decode on the host, pinned non-blocking uploads
            idx = missing[k:k + 16]
            up = ds._to_device_async(np.stack([ds._image(i) for i in idx]))
            if up.shape[1:] != dev.shape[1:]:
                raise ValueError(f"images of shape {tuple(up.shape[1:])} do not match the resident cache {tuple(dev.shape[1:])}")
            dev[ds._to_device_async(np.asarray(idx, np.int64))] = up
            have[idx] = True
            for i in idx:
                ds._cache.pop(i, None)
        return dev, cams

    def __iter__(self):
        from ..runtime import draw_ray_batch
        ds = self._images
        rank, world = ds._placement()
        rank_positions(0, self.rays_per_step, rank, world)      # divisibility, before anything is drawn
        dev, cams = self._resident_all()
        steps = self.schedule()
        if self._rg is None:
            self._rg = ds._rg_factory(rank)                    # the camera model of the image-mode dataset
        rg = self._rg
        if (rg.image_height, rg.image_width) != tuple(dev.shape[1:3]):
            raise ValueError(f"the ray generator's {rg.image_height} x {rg.image_width} pixels do not match the images' "
                             f"{dev.shape[1]} x {dev.shape[2]}")
        model = getattr(rg, "ray_model", None)                 # None: the plain rays through the plain entry point
        extra = {} if model is None else {"ray_model": model}
        if getattr(rg, "camera", None) is not None:            # a calibrated camera: knerf_draw_ray_batch_cam, row v for view v
            extra["camera"] = rg.camera

        def gen():
            for perm, step in steps:
                first, n = rank_positions(step, self.rays_per_step, rank, world)
                # the ranks share the seed (one permutation); the jitter stream is new for every batch and every rank
                stream = self._drawn * world + rank
                self._drawn += 1
                self.last_draw = (perm, first, n)              # what the batch just yielded holds: positions [first, first + n) of `perm`
                index = None
                if self._cameras is None and not self.alpha and self._depth is None:
                    o, d, t, target = draw_ray_batch(dev, cams, rg.focal_length, rg.near, rg.far, rg.n_sample, self.seed, perm, first, n,
                                                     noise_stream=stream, **extra)
                elif self._cameras is None:
                    import torch
                    o, d, t, target, index = draw_ray_batch(dev, cams, rg.focal_length, rg.near, rg.far, rg.n_sample, self.seed, perm,
                                                            first, n, noise_stream=stream, want_index=True, **extra)
                    if self.alpha:
                        target = torch.cat([target, dev.reshape(-1, 4)[index.to(torch.int64), 3:4]], dim=1)
                else:
                    import torch
                    now = self._cameras()
                    if tuple(now.shape) != tuple(cams.shape) or now.dtype != cams.dtype or now.device != cams.device:
                        raise ValueError(f"the camera provider returned {tuple(now.shape)} {now.dtype} on {now.device}; the dataset "
                                         f"draws from {tuple(cams.shape)} {cams.dtype} on {cams.device}")
                    o, d, t, target, index = draw_ray_batch(dev, now.contiguous(), rg.focal_length, rg.near, rg.far, rg.n_sample,
                                                            self.seed, perm, first, n, noise_stream=stream, want_index=True, **extra)
                    self.last_view = torch.div(index, self._rows * self._cols, rounding_mode="floor").to(torch.int32)
                    if self.alpha:
                        target = torch.cat([target, dev.reshape(-1, 4)[index.to(torch.int64), 3:4]], dim=1)
                if self._depth is not None:                    # the maps at the drawn pixels
                    at = index.to("cuda").long()
                    z, c = self._depth
                    self.last_depth = (z.reshape(-1)[at], None if c is None else c.reshape(-1)[at])
                else:
                    self.last_depth = None
                yield target, (o, d, t)
        return gen()
