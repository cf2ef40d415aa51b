"""Depth targets for the grid optimisers' depth_loss= keyword.  Extension, no reference counterpart.

The optimisers compare a ray's expected depth Z = sum w_j t_j with a target in the SAME unit: the parameter t along the direction
vector d the project's own ray kernels write for the pixel, so that the point is o + t d.  d is not normalised (the plain pinhole rays
have d_z = -1 in the camera's frame, a fisheye's have unit length), so neither a z-depth map nor a map of Euclidean distances is in
that unit by itself:

  ray_parameter_from_z         dense z-depth (the distance along the camera's viewing axis, what RGB-D sensors and most renderers store)
  ray_parameter_from_distance  dense Euclidean distance from the camera centre
  sparse_depth_maps            structure-from-motion points (COLMAP's points3D) -> sparse maps [V,H,W] with DS-NeRF's weights

The first two are elementwise and take NumPy arrays or torch tensors; the third runs in torch on the device (CameraModel.project and the
dataset's own ray generator: set-up work, no kernel of its own)."""
from __future__ import annotations

import numpy as np


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch")


def ray_parameter_from_distance(dist, directions):
    """t = dist / |d|: Euclidean distances [...] from the ray origins and the rays' direction vectors [..., 3] -> ray parameters [...]"""
    if _is_tensor(dist) or _is_tensor(directions):
        import torch
        d = torch.as_tensor(directions)
        dist = torch.as_tensor(dist).to(d.device)
        if d.shape[-1] != 3 or tuple(d.shape[:-1]) != tuple(dist.shape):
            raise ValueError(f"directions must be {tuple(dist.shape)} + (3,), got {tuple(d.shape)}")
        return dist / torch.sqrt((d * d).sum(dim=-1))
    d, dist = np.asarray(directions), np.asarray(dist)
    if d.shape[-1:] != (3,) or d.shape[:-1] != dist.shape:
        raise ValueError(f"directions must be {dist.shape} + (3,), got {d.shape}")
    return dist / np.sqrt((d * d).sum(axis=-1))


def ray_parameter_from_z(z, directions, c2w):
    """t = z / (d . f): z-depths [...] (distance along the viewing axis f = -c2w[:3, 2]: this project's cameras look along -z), the rays'
    direction vectors [..., 3] and the camera-to-world matrix [4,4] -- or [V,4,4] for maps [V, ...], one camera per leading index ->
    ray parameters [...]"""
    if _is_tensor(z) or _is_tensor(directions) or _is_tensor(c2w):
        import torch
        d = torch.as_tensor(directions)
        z, m = torch.as_tensor(z).to(d.device), torch.as_tensor(c2w).to(d.device, d.dtype)
        xp_sum = lambda a: a.sum(dim=-1)
    else:
        d, z, m = np.asarray(directions), np.asarray(z), np.asarray(c2w)
        xp_sum = lambda a: a.sum(axis=-1)
    if tuple(d.shape[-1:]) != (3,) or tuple(d.shape[:-1]) != tuple(z.shape):
        raise ValueError(f"directions must be {tuple(z.shape)} + (3,), got {tuple(d.shape)}")
    if tuple(m.shape) == (4, 4):
        f = -m[:3, 2]
    elif len(m.shape) == 3 and tuple(m.shape[1:]) == (4, 4) and len(z.shape) >= 1 and m.shape[0] == z.shape[0]:
        f = (-m[:, :3, 2]).reshape((m.shape[0],) + (1,) * (len(z.shape) - 1) + (3,))
    else:
        raise ValueError(f"c2w must be [4,4], or [V,4,4] with V = {z.shape[0] if len(z.shape) else 1} maps; got {tuple(m.shape)}")
    return z / xp_sum(d * f)


def point_weights(errors):
    """exp(-(err / mean err)^2): the confidence DS-NeRF gives a structure-from-motion point of reprojection error err (float64 [P])"""
    e = np.asarray(errors, np.float64).reshape(-1)
    if e.size == 0 or not np.all(np.isfinite(e)) or np.any(e < 0):
        raise ValueError("errors must be a non-empty array of finite reprojection errors >= 0")
    mean = e.mean()
    return np.exp(-(e / mean) ** 2) if mean > 0 else np.ones_like(e)


def sparse_depth_maps(points, errors, tracks, dataset, views):
    """Sparse depth maps from structure-from-motion points, on the device: (depth [V,H,W], weight [V,H,W]) float32 for the V views of
    `dataset` (a RayImageDataset), in the unit the grid optimisers take.
      points [P,3]   world coordinates, in the units of the dataset's poses
      errors [P]     reprojection errors (any unit: only err / mean err enters)
      tracks         per point, the ids of the images that observe it
      views          the image id of every view of the dataset, in the dataset's order; observations by other images are dropped
    Every observation is projected with the dataset's camera (CameraModel.project) and lands on the nearest pixel (row, col); with
    (o, d) that pixel's ray from the dataset's own ray generator, t* = (X - o) . d / (d . d).  A point behind its camera or outside the
    image is dropped; the nearest t* wins where points share a pixel; weight = point_weights(errors) of the winner.  Pixels without a
    point have weight 0 (and depth 0).  ValueError for NDC rays: their parameter is not a depth of the scene."""
    import torch
    from .cameras import CameraModel
    from .raybatch import loader_output_size
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    wts = point_weights(errors)
    if len(tracks) != pts.shape[0] or wts.shape[0] != pts.shape[0]:
        raise ValueError(f"{pts.shape[0]} points, {wts.shape[0]} errors and {len(tracks)} tracks")
    view_of = {int(image_id): v for v, image_id in enumerate(views)}
    V = len(dataset.image_paths)
    if len(view_of) != V:
        raise ValueError(f"views names {len(view_of)} distinct images for a dataset of {V} views")
    rg = dataset._rg_factory(dataset._placement()[0])        # a generator of its own: the dataset's jitter streams are not advanced
    if getattr(rg, "ndc", False):
        raise ValueError("sparse depth under NDC rays is not supported: an NDC ray's parameter is not a depth of the scene")
    H, W = loader_output_size(dataset.image_loader)
    if (rg.image_height, rg.image_width) != (H, W):
        raise ValueError(f"the ray generator's {rg.image_height} x {rg.image_width} pixels do not match the images' {H} x {W}")
    pi, vi = [], []
    for p, track in enumerate(tracks):
        for v in sorted({view_of[int(i)] for i in track if int(i) in view_of}):
            pi.append(p); vi.append(v)
    depth = torch.zeros((V, H, W), device="cuda", dtype=torch.float32)
    weight = torch.zeros((V, H, W), device="cuda", dtype=torch.float32)
    if not pi:
        return depth, weight
    camera = rg.camera if getattr(rg, "camera", None) is not None else CameraModel.from_focal(rg.focal_length, W, H)
    c2w = torch.as_tensor(np.stack(dataset.camera_params).astype(np.float32)).to("cuda")
    pi_t, vi_t = torch.as_tensor(np.asarray(pi, np.int64)).to("cuda"), torch.as_tensor(np.asarray(vi, np.int64)).to("cuda")
    X = torch.as_tensor(pts).to("cuda")[pi_t]                                # float64 [n,3]
    pix, _, valid = camera.project(X.to(torch.float32), c2w, view=vi_t)
    col, row = torch.round(pix[:, 0]).to(torch.int64), torch.round(pix[:, 1]).to(torch.int64)
    keep = valid.bool() & torch.isfinite(pix).all(dim=1) & (col >= 0) & (col < W) & (row >= 0) & (row < H)
    # the rays of every view, one view per launch (a per-view camera takes its row by view_index)
    per_view = getattr(rg, "camera", None) is not None and rg.camera.n_cameras > 1
    o = torch.empty((V, H, W, 3), device="cuda", dtype=torch.float32)
    d = torch.empty_like(o)
    for v in range(V):
        o[v], d[v], _ = rg(c2w[v], **({"view_index": [v]} if per_view else {}))
    flat = ((vi_t * H + row.clamp(0, H - 1)) * W + col.clamp(0, W - 1))[keep]
    oo, dd = o.reshape(-1, 3)[flat].to(torch.float64), d.reshape(-1, 3)[flat].to(torch.float64)
    t = ((X[keep] - oo) * dd).sum(dim=1) / (dd * dd).sum(dim=1)
    ahead = t > 0
    flat, t, w = flat[ahead], t[ahead].to(torch.float32), torch.as_tensor(wts).to("cuda")[pi_t[keep][ahead]].to(torch.float32)
    nearest = torch.full((V * H * W,), float("inf"), device="cuda", dtype=torch.float32)
    nearest.scatter_reduce_(0, flat, t, "amin")
    won = t == nearest[flat]
    weight.reshape(-1).scatter_reduce_(0, flat[won], w[won], "amax")         # (equal depths on one pixel: the more trusted point)
    hit = torch.isfinite(nearest)
    depth.reshape(-1)[hit] = nearest[hit]
    return depth, weight
