"""fp64 NumPy restatements of the forward-facing ray stage (csrc/rays_ext.h) and of the LLFF pose
normalisation (keras_nerf_amd/data/llff.py): the specifications the kernels and the loader are tested against.  Plus the small LLFF
directory and the camera poses the tests share."""
import os

import numpy as np


def ndc_rays(o, d, focal, W, H, n=1.0):
    """pinhole rays o, d [...,3] of cameras that look along -z -> (o' [...,3], unit d' / L [...,3], L [...]) in NDC space with the
    near plane at distance n"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    s = -(n + o[..., 2]) / d[..., 2]
    o = o + s[..., None] * d
    ax, ay = -(2.0 * focal / W), -(2.0 * focal / H)
    o2 = np.stack([ax * o[..., 0] / o[..., 2], ay * o[..., 1] / o[..., 2], 1.0 + 2.0 * n / o[..., 2]], -1)
    d2 = np.stack([ax * (d[..., 0] / d[..., 2] - o[..., 0] / o[..., 2]), ay * (d[..., 1] / d[..., 2] - o[..., 1] / o[..., 2]),
                   -2.0 * n / o[..., 2]], -1)
    L = np.linalg.norm(d2, axis=-1)
    return o2, d2 / L[..., None], L


def perspective(p, focal, W, H, n=1.0):
    """the perspective map of world points p [...,3] that NDC rays are straight lines under"""
    p = np.asarray(p, np.float64)
    return np.stack([-(2.0 * focal / W) * p[..., 0] / p[..., 2], -(2.0 * focal / H) * p[..., 1] / p[..., 2], 1.0 + 2.0 * n / p[..., 2]], -1)


def stratified(N, near, far, u):
    """rays.h stratified_sample in fp64: clip(linspace(near, far, N) + u * interval - interval / 2, near, far), u [...,N]"""
    u = np.asarray(u, np.float64)
    interval = (far - near) / N
    return np.clip(np.linspace(near, far, N) + u * interval - interval / 2.0, near, far)


def disparity_samples(N, near, far, u):
    """t = 1 / ((1 - s) / near + s / far), s the stratified sample on [0, 1]"""
    s = stratified(N, 0.0, 1.0, u)
    return 1.0 / ((1.0 - s) / near + s / far)


def ndc_samples(N, near, far, u, L):
    """t = s L, s the stratified sample on [near, far] inside [0, 1]; L [...]"""
    return stratified(N, near, far, u) * np.asarray(L, np.float64)[..., None]


# ---- the LLFF pose normalisation
def llff_axes(raw):
    """raw [V,3,5] as stored (columns: down, right, backwards, translation, hwf) -> [V,3,4] in (right, up, backwards)"""
    raw = np.asarray(raw, np.float64)
    return np.stack([raw[:, :, 1], -raw[:, :, 0], raw[:, :, 2], raw[:, :, 3]], -1)


def average_pose(poses):
    """4x4: centre = mean translation, z = normalised sum of the z columns, up = sum of the y columns, x = normalise(up x z), y = z x x"""
    p = np.asarray(poses, np.float64)
    z = p[:, :3, 2].sum(0); z /= np.linalg.norm(z)
    x = np.cross(p[:, :3, 1].sum(0), z); x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, p[:, :3, 3].mean(0)
    return m


def normalised_poses(poses_bounds, bd_factor=0.75, recenter=True):
    """poses_bounds [V,17] -> (poses [V,4,4] in (right, up, backwards), scaled and recentred; bounds [V,2] scaled)"""
    arr = np.asarray(poses_bounds, np.float64)
    p34 = llff_axes(arr[:, :15].reshape(-1, 3, 5))
    bounds = arr[:, 15:].copy()
    sc = 1.0 / (bounds.min() * bd_factor)
    p34[:, :, 3] *= sc
    bounds *= sc
    poses = np.tile(np.eye(4), (len(p34), 1, 1))
    poses[:, :3] = p34
    if recenter:
        poses = np.linalg.inv(average_pose(poses)) @ poses
    return poses, bounds


# ---- shared fixtures
GPU_POSE_SEED = 7        # random_poses(3, GPU_POSE_SEED): the cameras of tests/test_gpu_forward_facing.py


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def random_poses(V, seed=0, angle=0.35, shift=0.5):
    """[V,4,4] float32 camera-to-world (right, up, backwards): rotations within +-angle rad about each axis, translations within +-shift"""
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4), (V, 1, 1))
    for v in range(V):
        out[v, :3, :3] = rotation(*rng.uniform(-angle, angle, 3))
        out[v, :3, 3] = rng.uniform(-shift, shift, 3)
    return out.astype(np.float32)


def write_llff(root, V=10, H=12, W=20, focal=18.0, seed=0, factors=(1,), suffix=".png"):
    """a small LLFF directory: V views of H x W images (and reduced copies images_{f} for further factors), a seeded
    poses_bounds.npy with depth bounds around [2, 12].  Returns (root, poses_bounds [V,17])."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    c2w = random_poses(V, seed=seed + 1).astype(np.float64)
    c2w[:, :3, 3] += np.array([0.3, -0.2, 0.4])            # an average pose away from the identity
    rows = []
    for v in range(V):
        R, t = c2w[v, :3, :3], c2w[v, :3, 3]
        stored = np.stack([-R[:, 1], R[:, 0], R[:, 2], t, np.array([H, W, focal], np.float64)], -1)     # (down, right, backwards)
        rows.append(np.concatenate([stored.reshape(-1), [2.0 + rng.uniform(0, 0.5), 12.0 + rng.uniform(0, 3.0)]]))
    pb = np.stack(rows)
    os.makedirs(root, exist_ok=True)
    np.save(os.path.join(root, "poses_bounds.npy"), pb)
    for f in factors:
        folder = os.path.join(root, "images" if f == 1 else f"images_{f}")
        os.makedirs(folder, exist_ok=True)
        for v in range(V):
            img = rng.integers(0, 256, (H // f, W // f, 3), dtype=np.uint8)
            Image.fromarray(img, "RGB").save(os.path.join(folder, f"view_{v:03d}{suffix}"))
    return root, pb
