"""DatasetLoader -- counterpart of reference keras_nerf/data/loader.py:12-113 for nerf_synthetic-layout directories.

`load_dataset(...)` returns [train, val, test]; each is a re-iterable `RayImageDataset` that yields
(images [B,H,W,4] float32, (ray_origin [B,H,W,3], ray_direction [B,H,W,3], sample_points [B,H,W,N])) exactly like the
reference's zipped/shuffled/batched tf.data pipeline: shuffle with a buffer of `batch_size` elements, batches of
`batch_size`, remainder dropped, ray jitter redrawn on every pass (the tf.data `map` re-executes per epoch).
Images are decoded on the host (ImageLoader); rays are generated on the GPU (RaysGenerator).

Data parallel (one process per GPU, reference train.py:75-93): the reference builds ONE dataset with the GLOBAL batch
(`load_dataset(batch_size=args.batch_size * strategy.num_replicas_in_sync)`, train.py:84-93) and Keras hands replica r images
[r*b, (r+1)*b) of every global batch (b = args.batch_size, what NeRF.compile and NeRFTrainMonitor are given).  Same here, so that
an import-swapped train.py needs no change: `batch_size` IS THE GLOBAL BATCH; inside a torch.distributed job of W ranks every
rank builds the same dataset, all ranks draw the same shuffled order (one shared seed, shuffle buffer = the global batch as in
loader.py:97-113), cut it into global batches (remainder dropped) and yield their own slice of batch_size / W images (W must divide
it), so the replicas see disjoint images and the SUM all-reduce of NeRF.train_step adds gradients of different data.  The ray
jitter stream is keyed by the rank as well.  (Rounds 1-4 took the per-replica batch here; train.py passes the global one.)

Feeding the GPU (the reference prefetches with tf.data, loader.py:104-106): the decoded images and the camera matrices of a
dataset are kept RESIDENT ON THE DEVICE (100 views of 800 x 800 x 4 floats are 1 GB of 288), filled as the first pass touches
them, so from the second epoch on a batch is one gather on the device plus the ray-generation kernel -- no host-to-device copy
and, above all, no pageable copy that would make the host wait for the previous train step.  The few indices a batch needs
travel through pinned memory with a non-blocking copy.  A dataset larger than `device_cache_gb` (default 64) is staged through
two pinned buffers on a side stream instead, one batch ahead of the step that consumes it.

`RayImageDataset.ray_batches(rays_per_step)` gives the same data as batches of rays drawn at random over all pixels of all images
(raybatch.py): the usual way to train a NeRF, which the reference does not have.

A `transforms_*.json` that carries the nerfstudio / instant-ngp intrinsics (fl_x, fl_y, cx, cy, w, h, distortion coefficients,
camera_model; at top level or per frame) is loaded with a calibrated camera (`camera_from_transforms`, data/cameras.py); a file
without them loads exactly as the reference loads it."""
from __future__ import annotations

import json
import logging
import os
from typing import List

import numpy as np

from .image import ImageLoader
from .utils import get_focal_from_fov


class _Iterator:
    def __init__(self, it):
        self._it = it

    def get_next(self):
        return next(self._it)

    __next__ = get_next

    def __iter__(self):
        return self


def _dist_rank_world():
    """(rank, world size) of the torch.distributed job this process belongs to, (0, 1) outside one"""
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except Exception:
        pass
    return 0, 1


def shuffled_order(n, buffer_size, rng):
    """tf.data shuffle(buffer_size): keep a buffer of `buffer_size` elements, emit a random one, refill in order"""
    buf, out, nxt = [], [], 0
    while nxt < n or buf:
        while nxt < n and len(buf) < buffer_size:
            buf.append(nxt); nxt += 1
        out.append(buf.pop(int(rng.integers(len(buf)))))
    return out


def replica_batches(order, batch_size, rank=0, world=1, limit=None):
    """index lists of this replica's batches: `order` cut into global batches of batch_size x world (drop_remainder=True),
    replica r keeps elements [r*b, (r+1)*b) of each (train.py:84-93: Keras splits the global batch along dim 0)"""
    g = batch_size * world
    nb = len(order) // g
    if limit is not None:
        nb = min(nb, limit)
    return [order[k * g + rank * batch_size:k * g + (rank + 1) * batch_size] for k in range(nb)]


class RayImageDataset:
    def __init__(self, image_paths, camera_params, image_loader, rays_generator_factory, batch_size, seed=0, limit=None,
                 rank=None, world=None, device_cache_gb=64.0, _shared=None):
        """rank / world: data-parallel placement; None = taken from torch.distributed when an iteration starts.
        device_cache_gb: keep the whole dataset on the device when it fits this budget (see the module docstring)."""
        self.image_paths, self.camera_params = list(image_paths), [np.asarray(c, np.float32) for c in camera_params]
        self.image_loader, self._rg_factory, self._rg = image_loader, rays_generator_factory, None
        self.batch_size, self._rng, self._limit = batch_size, np.random.default_rng(seed), limit
        self._rank, self._world = rank, world
        self.device_cache_gb = device_cache_gb
        # decoded host images and the device-resident copies are shared between a dataset and its take() views
        self._shared = _shared if _shared is not None else {"host": {}, "dev": None, "have": None, "cams": None}
        self._cache = self._shared["host"]

    def _placement(self):
        if self._rank is not None and self._world is not None:
            return self._rank, self._world
        return _dist_rank_world()

    def _local_batch(self, world):
        """images per step of ONE replica: the global batch split along dim 0 (train.py:84-93)"""
        if self.batch_size % world:
            raise ValueError(f"the global batch of {self.batch_size} images is not divisible by {world} replicas "
                             f"(train.py:84: global_batch_size = batch_size x num_replicas_in_sync)")
        return self.batch_size // world

    def __len__(self):
        n = len(self.image_paths) // self.batch_size          # global batches; every replica takes part in each
        return n if self._limit is None else min(n, self._limit)

    def take(self, n):
        return RayImageDataset(self.image_paths, self.camera_params, self.image_loader, self._rg_factory, self.batch_size,
                               seed=int(self._rng.integers(1 << 31)), limit=n, rank=self._rank, world=self._world,
                               device_cache_gb=self.device_cache_gb, _shared=self._shared)

    def private_view(self, seed=0, limit=None):
        """the same data behind an INDEPENDENT shuffle stream: iterating the view never advances this dataset's generator.
        For consumers that iterate on one rank only (NeRFTrainMonitor on rank 0), so that the ranks' shared order of THIS
        dataset stays in lock-step."""
        return RayImageDataset(self.image_paths, self.camera_params, self.image_loader, self._rg_factory, self.batch_size,
                               seed=seed, limit=self._limit if limit is None else limit, rank=self._rank, world=self._world,
                               device_cache_gb=self.device_cache_gb, _shared=self._shared)

    def ray_batches(self, rays_per_step, seed=0, steps_per_epoch=None, alpha=False, depth=None, depth_weight=None):
        """the same data as batches of `rays_per_step` rays drawn at random over all pixels of all images, one permutation of the
        pixels per epoch (raybatch.RayBatchDataset; needs the whole dataset within `device_cache_gb`).  Data parallel:
        `rays_per_step` is the GLOBAL count, every rank draws its 1/world slice of the same permutation.
        alpha=True: the targets are [n,4], the images' alpha as the fourth column (what the grid optimisers' background= and
        opacity_loss= keywords train against); without it the batches and the launches are what they were.
        depth, depth_weight: [V,H,W] maps of depth targets and weights (RayBatchDataset.set_depth; what the grid optimisers'
        depth_loss= keyword trains against); without them the batches and the launches are what they were."""
        from .raybatch import RayBatchDataset
        batches = RayBatchDataset(self, rays_per_step, seed=seed, steps_per_epoch=steps_per_epoch, alpha=alpha)
        if depth is not None or depth_weight is not None:
            batches.set_depth(depth, depth_weight)
        return batches

    def _image(self, i):
        if i not in self._cache:
            self._cache[i] = self.image_loader(self.image_paths[i])
        return self._cache[i]

    # ---- device-resident copy
    def _resident(self, shape):
        """(images [N,H,W,4], have [N] host bools, cams [N,4,4]) on the device, or None when the dataset exceeds the budget"""
        import torch
        sh = self._shared
        if sh["dev"] is None and sh.get("dev_refused") is None:
            n = len(self.image_paths)
            if n * int(np.prod(shape)) * 4 > self.device_cache_gb * 1e9:
                sh["dev_refused"] = True
            else:
                sh["dev"] = torch.empty((n, *shape), device="cuda", dtype=torch.float32)
                sh["have"] = np.zeros(n, bool)
                sh["cams"] = torch.as_tensor(np.stack(self.camera_params)).pin_memory().to("cuda", non_blocking=True)
        return None if sh["dev"] is None else (sh["dev"], sh["have"], sh["cams"])

    @staticmethod
    def _to_device_async(array):
        """small host array -> device without a pageable copy (which would make the host wait for the stream's earlier work)"""
        import torch
        return torch.as_tensor(array).pin_memory().to("cuda", non_blocking=True)

    def __iter__(self):
        import torch
        rank, world = self._placement()
        if self._rg is None:
            self._rg = self._rg_factory(rank)
        # the same order on every rank (the rngs are seeded alike and advance alike), each rank keeps its slice
        order = shuffled_order(len(self.image_paths), self.batch_size, self._rng)
        batches = replica_batches(order, self._local_batch(world), rank, world, self._limit)
        camera = getattr(self._rg, "camera", None)            # a per-view camera table: the generator is told each batch's views
        per_view = camera is not None and camera.n_cameras > 1
        if per_view and camera.n_cameras != len(self.image_paths):
            raise ValueError(f"the ray generator's camera has {camera.n_cameras} rows for {len(self.image_paths)} views")

        def gen_resident(res):
            dev, have, cams = res
            for idx in batches:
                missing = [i for i in idx if not have[i]]
                if missing:                                   # first touch: decode on the host, one pinned non-blocking upload
                    up = self._to_device_async(np.stack([self._image(i) for i in missing]))
                    dev[self._to_device_async(np.asarray(missing, np.int64))] = up
                    have[missing] = True
                    for i in missing:
                        self._cache.pop(i, None)              # the device copy is the cache now
                sel = self._to_device_async(np.asarray(idx, np.int64))
                o, d, t = self._rg(cams.index_select(0, sel), **({"view_index": sel} if per_view else {}))
                yield dev.index_select(0, sel), (o, d, t)

        def gen_staged():
            # two pinned staging buffers, copies on a side stream one batch ahead of the consumer
            side = torch.cuda.Stream()
            main = torch.cuda.current_stream()
            pinned, copied, pending = [None, None], [None, None], None

            def stage(k, idx):
                images = np.stack([self._image(i) for i in idx])
                if copied[k] is not None:
                    copied[k].synchronize()                   # the buffer's previous upload (two batches ago) has left it
                if pinned[k] is None or pinned[k].shape != images.shape:
                    pinned[k] = torch.empty(images.shape, dtype=torch.float32).pin_memory()
                pinned[k].copy_(torch.as_tensor(images))
                with torch.cuda.stream(side):
                    dev = pinned[k].to("cuda", non_blocking=True)
                    ev = torch.cuda.Event(); ev.record(side)
                copied[k] = ev
                return dev, ev
            for n, idx in enumerate(batches):
                cur = pending if pending is not None else stage(n & 1, idx)
                pending = stage((n + 1) & 1, batches[n + 1]) if n + 1 < len(batches) else None
                dev, ev = cur
                main.wait_event(ev)
                dev.record_stream(main)
                o, d, t = self._rg(self._to_device_async(np.stack([self.camera_params[i] for i in idx])),
                                   **({"view_index": self._to_device_async(np.asarray(idx, np.int64))} if per_view else {}))
                yield dev, (o, d, t)

        if not batches:
            return _Iterator(iter(()))
        res = self._resident(self._image(batches[0][0]).shape)
        return _Iterator(gen_resident(res) if res is not None else gen_staged())


INTRINSIC_KEYS = ("fl_x", "fl_y", "cx", "cy", "w", "h", "k1", "k2", "k3", "k4", "p1", "p2", "camera_model")
IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg")


def camera_from_transforms(cfg: dict, image_width: int, image_height: int):
    """The CameraModel (data/cameras.py) of a transforms file that carries the nerfstudio / instant-ngp intrinsics -- fl_x, fl_y, cx,
    cy, w, h, optionally k1, k2, k3, k4, p1, p2 and camera_model "OPENCV" | "OPENCV_FISHEYE", at top level (one camera) or per frame
    (a frame's keys override the top level; one camera per view) -- scaled from w x h to the requested size, rays through the pixel
    centres (pixel_offset 0.5).  None for a file without fl_x anywhere: the plain camera of camera_angle_x."""
    from .cameras import CameraModel
    frames = cfg.get("frames", [])
    if "fl_x" not in cfg and not any("fl_x" in fr for fr in frames):
        return None
    per_frame = any(key in fr for fr in frames for key in INTRINSIC_KEYS)
    rows = []
    for n, fr in enumerate(frames if per_frame else [{}]):
        g = {key: fr.get(key, cfg.get(key)) for key in INTRINSIC_KEYS}
        where = f"frame {n}" if per_frame else "the file"
        if g["fl_x"] is None or g["w"] is None or g["h"] is None:
            raise ValueError(f"{where}: fl_x, w and h are needed to state a camera")
        name = g["camera_model"]
        if name not in (None, "OPENCV", "OPENCV_FISHEYE", "PINHOLE", "SIMPLE_PINHOLE"):
            raise ValueError(f"{where}: camera_model {name!r} is not supported (OPENCV, OPENCV_FISHEYE)")
        k = {key: float(g[key] or 0.0) for key in ("k1", "k2", "k3", "k4", "p1", "p2")}
        if name == "OPENCV_FISHEYE":
            model, dist = "fisheye", (k["k1"], k["k2"], k["k3"], k["k4"])
        elif any(k[key] != 0.0 for key in ("k1", "k2", "k3", "p1", "p2")):
            model, dist = "opencv", (k["k1"], k["k2"], k["p1"], k["p2"], k["k3"])
        else:
            model, dist = "pinhole", ()
        w, h = float(g["w"]), float(g["h"])
        fl_x = float(g["fl_x"])
        rows.append((model, fl_x, float(g["fl_y"] if g["fl_y"] is not None else fl_x), float(g["cx"] if g["cx"] is not None else w / 2),
                     float(g["cy"] if g["cy"] is not None else h / 2), dist, image_width / w, image_height / h))
    models = {r[0] for r in rows} - {"pinhole"}
    if len(models) > 1:
        raise ValueError("a file that mixes OPENCV and OPENCV_FISHEYE cameras: one launch draws rays of one model")
    model = models.pop() if models else "pinhole"
    n_coeff = {"pinhole": 0, "opencv": 5, "fisheye": 4}[model]
    dist = np.array([list(r[5]) + [0.0] * (n_coeff - len(r[5])) for r in rows], np.float64).reshape(len(rows), n_coeff)
    col = lambda i, j: np.array([r[i] * r[j] for r in rows])
    return CameraModel(model, col(1, 6), col(2, 7), col(3, 6), col(4, 7), dist, pixel_offset=0.5)


class DatasetLoader:
    def __init__(self, data_dir: str, white_background: bool = False, **kwargs):
        self.data_dir, self.white_background = data_dir, white_background

    def _load_json(self, filename: str) -> dict:
        with open(filename, "r") as f:
            return json.load(f)

    def _load_image_path_and_camera_param(self, json_config: dict) -> tuple:
        paths = [os.path.join(self.data_dir, f"{fr['file_path']}.png") for fr in json_config["frames"]]
        return paths, [fr["transform_matrix"] for fr in json_config["frames"]]

    def _calibrated_dataset(self, cfg, camera, k, batch_size, image_width, image_height, near, far, n_sample):
        """the dataset of a file with intrinsics (camera_from_transforms): images resized to image_height rows x image_width columns
        (calibrated photographs are rarely square), file paths taken with their suffix when they have one"""
        loader = ImageLoader(image_width, image_height, self.white_background, height_first=True)

        def factory(rank=0):
            from .rays import RaysGenerator
            return RaysGenerator(focal_length=None, image_width=image_width, image_height=image_height, near=near, far=far,
                                 n_sample=n_sample, seed=1000 + k + 4096 * rank, camera=camera)
        paths = [os.path.join(self.data_dir, fr["file_path"] if fr["file_path"].lower().endswith(IMAGE_SUFFIXES) else f"{fr['file_path']}.png")
                 for fr in cfg["frames"]]
        return RayImageDataset(paths, [fr["transform_matrix"] for fr in cfg["frames"]], loader, factory, batch_size, seed=k)

    def load_dataset(self, batch_size: int, image_width: int, image_height: int, near: float, far: float, n_sample: int) -> List[RayImageDataset]:
        """loader.py:55-113.  batch_size: the GLOBAL batch (train.py:84-93 passes batch_size x replicas; train_single.py:60-67 the
        only batch there is); a rank of a data-parallel job yields its 1/world slice of every batch"""
        image_loader = ImageLoader(image_width, image_height, self.white_background)
        out = []
        self.cameras = []                                     # per subset: the CameraModel of a calibrated file, else None
        for k, subset in enumerate(["train", "val", "test"]):
            cfg = self._load_json(os.path.join(self.data_dir, f"transforms_{subset}.json"))
            camera = camera_from_transforms(cfg, image_width, image_height)
            self.cameras.append(camera)
            if camera is not None:
                camera.check_invertible(image_width, image_height)          # on the host, before anything is uploaded
                out.append(self._calibrated_dataset(cfg, camera, k, batch_size, image_width, image_height, near, far, n_sample))
                logging.info(f"Loaded {subset} dataset. {len(cfg['frames'])} images, {camera.model} camera.")
                continue
            focal = get_focal_from_fov(cfg["camera_angle_x"], image_width)

            def factory(rank=0, focal=focal, k=k):
                from .rays import RaysGenerator
                return RaysGenerator(focal_length=focal, image_width=image_width, image_height=image_height, near=near, far=far,
                                     n_sample=n_sample, seed=1000 + k + 4096 * rank)       # replicas jitter differently
            paths, cams = self._load_image_path_and_camera_param(cfg)
            out.append(RayImageDataset(paths, cams, image_loader, factory, batch_size, seed=k))
            logging.info(f"Loaded {subset} dataset. {len(paths)} images.")
        return out
