"""Camera helpers (host side, float32 NumPy): the public names and conventions of the reference's keras_nerf/data/utils.py
(focal length from the field of view at :5-16, the spherical camera pose at :52-63) on a small homogeneous-matrix toolkit."""
from __future__ import annotations

import numpy as np

_F = np.float32


def get_focal_from_fov(field_of_view: float, width: int) -> float:
    """focal = (width / 2) / tan(fov / 2), evaluated in float32 as the reference does"""
    half_width, half_fov = _F(0.5) * _F(width), _F(0.5) * _F(field_of_view)
    return float(half_width / np.tan(half_fov))


def _homogeneous(rotation=None, translation=(0.0, 0.0, 0.0)) -> np.ndarray:
    m = np.eye(4, dtype=_F)
    if rotation is not None:
        m[:3, :3] = rotation
    m[:3, 3] = translation
    return m


def _axis_rotation(axis: int, angle) -> np.ndarray:
    """3x3 rotation that leaves coordinate `axis` alone; on the two remaining coordinates (in increasing order) it is
    [[c, -s], [s, c]] -- the convention of both of the reference's rotation helpers"""
    c, s = np.cos(_F(angle)), np.sin(_F(angle))
    i, j = [k for k in range(3) if k != axis]
    r = np.eye(3, dtype=_F)
    r[i, i] = r[j, j] = c
    r[i, j], r[j, i] = -s, s
    return r


def get_translation_t(t):
    """camera pushed back by t along +z"""
    return _homogeneous(translation=(0.0, 0.0, t))


def get_rotation_phi(phi):
    """elevation: rotation about x (rows y,z = [c -s; s c])"""
    return _homogeneous(_axis_rotation(0, phi))


def get_rotation_theta(theta):
    """azimuth: rotation about y with the reference's sign (rows x,z = [c -s; s c])"""
    return _homogeneous(_axis_rotation(1, theta))


# world-from-blender axis swap applied last: x -> -x, y <-> z
_SWAP = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], _F)


def pose_spherical(theta, phi, t):
    """camera-to-world matrix of a camera at radius t looking at the origin, azimuth theta and elevation phi in degrees"""
    pose = get_translation_t(t)
    for rot, deg in ((get_rotation_phi, phi), (get_rotation_theta, theta)):
        pose = rot(deg / 180.0 * np.pi) @ pose
    return (_SWAP @ pose).astype(_F)


# ---- forward-facing captures (data/llff.py): pose normalisation and the spiral render path of the LLFF convention.  Poses are
# camera-to-world [..., 3 or 4, 4] in axes (right, up, backwards); everything here is evaluated in float64.
def _normalize(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _view_matrix(z, up, position) -> np.ndarray:
    """4x4 camera-to-world of a camera at `position` whose backwards axis is z, with `up` fixing the roll"""
    z = _normalize(z)
    x = _normalize(np.cross(up, z))
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, position
    return m


def poses_avg(poses) -> np.ndarray:
    """the average pose (4x4, float64): centre = mean translation, z = normalised sum of the z columns, up = sum of the y columns,
    x = normalise(up x z), y = z x x"""
    p = np.asarray(poses, np.float64)
    return _view_matrix(p[:, :3, 2].sum(0), p[:, :3, 1].sum(0), p[:, :3, 3].mean(0))


def recenter_poses(poses) -> np.ndarray:
    """every pose multiplied by the inverse of the average pose, [V,4,4] float64: the average of the result is the identity"""
    p = np.asarray(poses, np.float64)
    full = np.tile(np.eye(4), (p.shape[0], 1, 1))
    full[:, :3, :4] = p[:, :3, :4]
    return np.linalg.inv(poses_avg(p)) @ full


def render_path_spiral(poses, bounds, n_views=120, n_rots=2, zrate=0.5, rad_percentile=90, path_dt=0.75) -> np.ndarray:
    """[n_views,4,4] float32 camera poses on a spiral around the average pose, all looking at one focus point.
    focus depth = 1 / ((1 - dt) / (0.9 bounds.min()) + dt / (5 bounds.max())), dt = path_dt; radii = the `rad_percentile`-th percentile
    of |translation| per axis; view i at angle theta = 2 pi n_rots i / n_views looks from
    avg @ ([cos theta, -sin theta, -sin(theta zrate), 1] * [radii, 1]) at avg @ [0, 0, -focus, 1]."""
    p = np.asarray(poses, np.float64)
    b = np.asarray(bounds, np.float64)
    avg = poses_avg(p)
    up = _normalize(p[:, :3, 1].sum(0))
    dt = float(path_dt)
    focus = 1.0 / ((1.0 - dt) / (0.9 * b.min()) + dt / (5.0 * b.max()))
    rads = np.append(np.percentile(np.abs(p[:, :3, 3]), rad_percentile, axis=0), 1.0)
    target = avg[:3] @ np.array([0.0, 0.0, -focus, 1.0])
    out = []
    for theta in np.linspace(0.0, 2.0 * np.pi * n_rots, int(n_views) + 1)[:-1]:
        c = avg[:3] @ (np.array([np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.0]) * rads)
        out.append(_view_matrix(c - target, up, c))
    return np.stack(out).astype(_F)
