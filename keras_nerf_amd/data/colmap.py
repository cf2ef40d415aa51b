"""ColmapDatasetLoader -- captures reconstructed with COLMAP, read from its TEXT model (`cameras.txt`, `images.txt`, optionally
`points3D.txt`; `colmap model_converter --output_type TXT` writes them).  Extension, no reference counterpart.

The layout (public; restated from COLMAP's documentation of its output format):
  cameras.txt   CAMERA_ID MODEL WIDTH HEIGHT PARAMS[]
                  SIMPLE_PINHOLE f cx cy | PINHOLE fx fy cx cy | SIMPLE_RADIAL f cx cy k | RADIAL f cx cy k1 k2
                  OPENCV fx fy cx cy k1 k2 p1 p2 | OPENCV_FISHEYE fx fy cx cy k1 k2 k3 k4
  images.txt    two lines per image: IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME, then its 2-D points (may be empty).  The pose is
                world-to-camera, x_cam = R(q) x_world + t, the camera looking along +z with y down; pixel centres at half-integers
  points3D.txt  POINT3D_ID X Y Z R G B ERROR TRACK[] as (IMAGE_ID, POINT2D_IDX)

`load_dataset` returns [train, val, test] `RayImageDataset`s like `DatasetLoader`; every `holdout`-th image (in name order) is held out
and serves as both val and test.  Poses are inverted and their y and z columns flipped to this project's (right, up, backwards);
intrinsics become a per-view `CameraModel` (data/cameras.py) with pixel_offset 0.5, scaled per camera to the requested size.  One
launch draws rays of one model, so a dataset that mixes pinhole cameras with one other class is promoted to that class with zero
coefficients and a dataset that mixes the opencv class with fisheye cameras is refused.  With points3D.txt, `bounds` [V,2] holds the
0.1 / 99.9 percentiles of the depths of the points each image observes (else None) and `bd_factor` scales the scene like the LLFF
loader does.  Intrinsics and distortion are stated, not refined."""
from __future__ import annotations

import logging
import os
from typing import List

import numpy as np

from .cameras import CameraModel
from .image import ImageLoader
from .loader import RayImageDataset

# model name -> (class, number of parameters, parameters -> (fx, fy, cx, cy, coefficients of the class))
COLMAP_MODELS = {
    "SIMPLE_PINHOLE": ("pinhole", 3, lambda p: (p[0], p[0], p[1], p[2], ())),
    "PINHOLE": ("pinhole", 4, lambda p: (p[0], p[1], p[2], p[3], ())),
    "SIMPLE_RADIAL": ("opencv", 4, lambda p: (p[0], p[0], p[1], p[2], (p[3], 0.0, 0.0, 0.0, 0.0))),
    "RADIAL": ("opencv", 5, lambda p: (p[0], p[0], p[1], p[2], (p[3], p[4], 0.0, 0.0, 0.0))),
    "OPENCV": ("opencv", 8, lambda p: (p[0], p[1], p[2], p[3], (p[4], p[5], p[6], p[7], 0.0))),
    "OPENCV_FISHEYE": ("fisheye", 8, lambda p: (p[0], p[1], p[2], p[3], (p[4], p[5], p[6], p[7]))),
}


def quaternion_matrix(qw, qx, qy, qz) -> np.ndarray:
    """the rotation of a (not necessarily unit) quaternion, Hamilton convention as COLMAP writes it"""
    q = np.array([qw, qx, qy, qz], np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def colmap_to_c2w(q, t) -> np.ndarray:
    """world-to-camera (qw, qx, qy, qz), t -> 4x4 camera-to-world in (right, up, backwards)"""
    R = quaternion_matrix(*q)
    m = np.eye(4)
    m[:3, :3] = R.T
    m[:3, 3] = -R.T @ np.asarray(t, np.float64)
    m[:3, 1] *= -1.0
    m[:3, 2] *= -1.0
    return m


def read_cameras(path: str) -> dict:
    """cameras.txt -> {camera id: (class, width, height, fx, fy, cx, cy, coefficients)}; unknown models are refused by name"""
    out = {}
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if w[1] not in COLMAP_MODELS:
                raise ValueError(f"{path}: camera {w[0]} uses the model {w[1]}, which is not supported (supported: {', '.join(COLMAP_MODELS)})")
            cls, n, unpack = COLMAP_MODELS[w[1]]
            params = [float(v) for v in w[4:]]
            if len(params) != n:
                raise ValueError(f"{path}: camera {w[0]} ({w[1]}) has {len(params)} parameters, expected {n}")
            out[int(w[0])] = (cls, int(w[2]), int(w[3]), *unpack(params))
    if not out:
        raise ValueError(f"{path} lists no camera")
    return out


def read_images(path: str) -> list:
    """images.txt -> [(image id, (qw, qx, qy, qz), (tx, ty, tz), camera id, name)] sorted by name"""
    with open(path) as f:
        lines = [ln.rstrip("\n") for ln in f if not ln.lstrip().startswith("#")]
    while lines and not lines[0].strip():
        lines.pop(0)
    out = []
    for ln in lines[0::2]:                      # every second line lists the image's 2-D points and may be empty
        w = ln.split()
        if not w:
            continue
        if len(w) < 10:
            raise ValueError(f"{path}: expected IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME, got {ln!r}")
        out.append((int(w[0]), tuple(float(v) for v in w[1:5]), tuple(float(v) for v in w[5:8]), int(w[8]), " ".join(w[9:])))
    if not out:
        raise ValueError(f"{path} lists no image")
    return sorted(out, key=lambda r: r[4])


def read_point_tracks(path: str) -> list:
    """points3D.txt -> [(xyz [3], [image ids])]"""
    out = []
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            out.append((np.array([float(v) for v in w[1:4]]), [int(v) for v in w[8::2]]))
    return out


def read_points(path: str):
    """points3D.txt -> (xyz float64 [P,3], error float64 [P], tracks: per point the int array of the ids of its observing images)"""
    xyz, err, tracks = [], [], []
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if len(w) < 8:
                raise ValueError(f"{path}: expected POINT3D_ID X Y Z R G B ERROR TRACK[], got {line.rstrip()!r}")
            xyz.append([float(v) for v in w[1:4]])
            err.append(float(w[7]))
            tracks.append(np.array([int(v) for v in w[8::2]], np.int64))
    return np.array(xyz, np.float64).reshape(-1, 3), np.array(err, np.float64), tracks


class ColmapDatasetLoader:
    def __init__(self, data_dir: str, model_dir: str = "sparse/0", images_dir: str = "images", holdout: int = 8, bd_factor: float = None,
                 white_background: bool = False, **kwargs):
        self.data_dir, self.model_dir, self.images_dir = data_dir, model_dir, images_dir
        self.holdout, self.bd_factor, self.white_background = int(holdout), bd_factor, white_background
        if self.holdout < 2:
            raise ValueError(f"holdout = {holdout}: every holdout-th view is held out, so it must be at least 2")
        if bd_factor is not None and not bd_factor > 0:
            raise ValueError(f"bd_factor = {bd_factor}: expected a positive number or None")
        self.poses = self.bounds = self.camera = self.image_paths = None
        self.image_ids, self.scale, self._subsets = None, 1.0, {}

    def _load_model(self, image_width: int, image_height: int):
        """sets image_paths, poses [V,4,4] float64, bounds [V,2] or None and the per-view camera at the requested size"""
        root = os.path.join(self.data_dir, self.model_dir)
        if not os.path.exists(os.path.join(root, "cameras.txt")):
            if os.path.exists(os.path.join(root, "cameras.bin")):
                raise ValueError(f"{root} holds COLMAP's binary model; export it as text first "
                                 f"(colmap model_converter --input_path {root} --output_path {root} --output_type TXT)")
            raise ValueError(f"{root} holds no cameras.txt")
        cameras = read_cameras(os.path.join(root, "cameras.txt"))
        images = read_images(os.path.join(root, "images.txt"))
        classes = {cameras[im[3]][0] for im in images} - {"pinhole"}
        if len(classes) > 1:
            raise ValueError("the dataset mixes cameras of the opencv class (SIMPLE_RADIAL, RADIAL, OPENCV) with OPENCV_FISHEYE: "
                             "one launch draws rays of one model")
        model = classes.pop() if classes else "pinhole"
        n_coeff = {"pinhole": 0, "opencv": 5, "fisheye": 4}[model]
        fx, fy, cx, cy, dist, w2c = [], [], [], [], [], {}
        poses = np.tile(np.eye(4), (len(images), 1, 1))
        for v, (image_id, q, t, cam_id, _name) in enumerate(images):
            if cam_id not in cameras:
                raise ValueError(f"image {image_id} names camera {cam_id}, which cameras.txt does not list")
            _cls, w, h, fx_, fy_, cx_, cy_, c = cameras[cam_id]
            sx, sy = image_width / w, image_height / h
            fx.append(fx_ * sx); fy.append(fy_ * sy); cx.append(cx_ * sx); cy.append(cy_ * sy)
            dist.append(list(c) + [0.0] * (n_coeff - len(c)))           # a pinhole camera promoted: zero coefficients
            poses[v] = colmap_to_c2w(q, t)
            w2c[image_id] = (v, quaternion_matrix(*q), np.asarray(t, np.float64))
        bounds = None
        pts = os.path.join(root, "points3D.txt")
        if os.path.exists(pts):
            depths = [[] for _ in images]
            for xyz, ids in read_point_tracks(pts):
                for image_id in set(ids):
                    if image_id in w2c:
                        v, R, t = w2c[image_id]
                        depths[v].append((R @ xyz + t)[2])
            if any(len(dv) == 0 for dv in depths):
                raise ValueError(f"{pts}: image {images[[len(dv) for dv in depths].index(0)][4]} observes no 3-D point")
            bounds = np.array([np.percentile(dv, [0.1, 99.9]) for dv in depths])
        if self.bd_factor is not None:
            if bounds is None:
                raise ValueError("bd_factor needs points3D.txt: the scale comes from the nearest depth bound")
            sc = 1.0 / (bounds.min() * self.bd_factor)
            poses[:, :3, 3] *= sc
            bounds = bounds * sc
            self.scale = float(sc)
        self.image_ids = [im[0] for im in images]
        self.image_paths = [os.path.join(self.data_dir, self.images_dir, im[4]) for im in images]
        self.poses, self.bounds = poses, bounds
        self.camera = CameraModel(model, fx, fy, cx, cy, np.array(dist, np.float64).reshape(len(images), n_coeff), pixel_offset=0.5)

    def split(self, n_views: int):
        """(train indices, held-out indices): every holdout-th view, starting with view 0, is held out"""
        held = [i for i in range(n_views) if i % self.holdout == 0]
        return [i for i in range(n_views) if i % self.holdout != 0], held

    def load_dataset(self, batch_size: int, image_width: int, image_height: int, near: float, far: float,
                     n_sample: int) -> List[RayImageDataset]:
        """[train, val, test]; batch_size is the GLOBAL batch as in DatasetLoader.load_dataset.  near, far: the sample range of every
        ray, in the (scaled) scene's units -- `bounds` says what each view sees"""
        self._load_model(image_width, image_height)
        self.camera.check_invertible(image_width, image_height)
        image_loader = ImageLoader(image_width, image_height, self.white_background, height_first=True)
        train_idx, held_idx = self.split(len(self.image_paths))
        out = []
        for k, (subset, idx) in enumerate([("train", train_idx), ("val", held_idx), ("test", held_idx)]):
            camera = self.camera.select(idx)

            def factory(rank=0, k=k, camera=camera):
                from .rays import RaysGenerator
                return RaysGenerator(focal_length=None, image_width=image_width, image_height=image_height, near=near, far=far,
                                     n_sample=n_sample, seed=1000 + k + 4096 * rank, camera=camera)     # replicas jitter differently
            out.append(RayImageDataset([self.image_paths[i] for i in idx], [self.poses[i].astype(np.float32) for i in idx],
                                       image_loader, factory, batch_size, seed=k))
            self._subsets[subset] = (out[-1], [self.image_ids[i] for i in idx])
            logging.info(f"Loaded {subset} dataset. {len(idx)} images, {self.camera.model} cameras.")
        return out

    def sparse_depth(self, subset: str = "train"):
        """(depth [V,H,W], weight [V,H,W]) float32 on the device for the views of a split of the last load_dataset(): the points of
        points3D.txt as depth targets for the grid optimisers' depth_loss= keyword, in their unit (data/depth.py sparse_depth_maps:
        every point lands on the nearest pixel of each image of its track, the nearest wins, weight exp(-(err / mean err)^2); pixels
        without a point have weight 0).  bd_factor's scale applies to the points as it does to the poses.  Feed them to
        ray_batches(n, depth=, depth_weight=).  ValueError before load_dataset(), for an unknown split and without points3D.txt."""
        from .depth import sparse_depth_maps
        if subset not in self._subsets:
            raise ValueError(f"subset = {subset!r}: load_dataset() first, then one of {sorted(self._subsets) or ['train', 'val', 'test']}")
        pts = os.path.join(self.data_dir, self.model_dir, "points3D.txt")
        if not os.path.exists(pts):
            raise ValueError(f"{pts} does not exist: sparse depth needs the model's points3D.txt")
        xyz, err, tracks = read_points(pts)
        if not len(err):
            raise ValueError(f"{pts} lists no point")
        dataset, ids = self._subsets[subset]
        return sparse_depth_maps(xyz * self.scale, err, tracks, dataset, ids)
