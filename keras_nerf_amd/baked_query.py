"""What a baked field holds at a point, and meshes from it: query, density_grid and extract_mesh for BakedField, BrickBakedField and
QuantizedBrickField, the counterparts of NeRF.query / NeRF.density_grid / NeRF.extract_mesh for a field that may have no MLP behind
it (extension, no reference counterpart).

The arithmetic is HIP (csrc/baked_query.hip: knerf_baked_query, knerf_baked_query_bricks, knerf_baked_query_qbricks; include/knerf.h
holds the specification, tests/baked_query_reference.py restates it in fp64): the renderer's evaluation of one sample, so a queried
sigma is the sigma the march composites at that position.  torch is used for device memory and streams, and for the copy of the stored
sigma column that density_grid() returns when it is asked for the lattice itself.  Every argument is checked on the host, before
anything touches the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .baked import LANES, BakedField, BrickBakedField, _brick_points_device, _brick_slabs, _check, _stream

MAX_GRID_POINTS = 1 << 31
MAX_POINTS = 1 << 36


def _storage(field):
    """(entry point, lanes per point the degree has) of a field's storage"""
    from .baked_quant import QLANES, QuantizedBrickField
    if isinstance(field, BakedField):
        return "knerf_baked_query", LANES[field.sh_degree]
    if isinstance(field, BrickBakedField):
        return "knerf_baked_query_bricks", LANES[field.sh_degree]
    if isinstance(field, QuantizedBrickField):
        return "knerf_baked_query_qbricks", QLANES[field.sh_degree]
    raise ValueError(f"need a BakedField, BrickBakedField or QuantizedBrickField, got {type(field).__name__}")


def _shape(x, what):
    """the shape of a tensor or of anything NumPy reads as an array of numbers, without moving it"""
    if hasattr(x, "shape") and hasattr(x, "dtype"):
        return tuple(int(s) for s in x.shape)
    try:
        return tuple(np.asarray(x, dtype=np.float32).shape)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be an array of numbers, got {type(x).__name__}") from None


def check_lanes(field, lanes_per_point) -> int:
    _, lanes = _storage(field)
    if isinstance(lanes_per_point, bool) or not isinstance(lanes_per_point, (int, np.integer)) or \
            (lanes_per_point != 0 and int(lanes_per_point) not in lanes):
        raise ValueError(f"lanes_per_point must be 0 (default) or one of {lanes} for a {type(field).__name__} of sh_degree "
                         f"{field.sh_degree}, got {lanes_per_point!r}")
    return int(lanes_per_point)


def check_query_args(field, points, directions=None, lanes_per_point=0):
    """NeRF.query's shape rules, on the host: points [..., 3]; directions None, 3 numbers in any shape (one shared direction) or
    something that broadcasts to the points' shape.  -> (leading shape, number of points, 0 | 1 | 3: no / one shared / per-point
    directions, lanes)"""
    lanes = check_lanes(field, lanes_per_point)
    ps = _shape(points, "points")
    if len(ps) < 1 or ps[-1] != 3:
        raise ValueError(f"points must have a last dimension of 3, got {ps}")
    n = int(np.prod(ps[:-1], dtype=np.int64)) if len(ps) > 1 else 1
    if n >= MAX_POINTS:
        raise ValueError(f"{n} points; at most 2^36 - 1 in one call")
    mode = 0
    if directions is not None:
        ds = _shape(directions, "directions")
        if len(ds) < 1 or ds[-1] != 3:
            raise ValueError(f"directions must have a last dimension of 3, got {ds}")
        mode = 1
        if int(np.prod(ds, dtype=np.int64)) != 3:
            try:
                ok = np.broadcast_shapes(ds, ps) == ps
            except ValueError:
                ok = False
            if not ok:
                raise ValueError(f"directions {ds} do not broadcast to the points' shape {ps}")
            mode = 3
    return ps[:-1], n, mode, lanes


def check_grid_args(field, resolution=None, bounds=None, direction=None):
    """NeRF.density_grid's rules with the field's own lattice and box as defaults -> (resolution, lo, hi, lattice): lattice = the grid
    asked for is the field's lattice itself (neither resolution nor bounds given)"""
    _storage(field)
    lattice = resolution is None and bounds is None
    if resolution is None:
        res = field.resolution
    else:
        res = (resolution,) * 3 if isinstance(resolution, (int, np.integer)) and not isinstance(resolution, bool) else \
            (tuple(resolution) if isinstance(resolution, (tuple, list, np.ndarray)) else ())
        if len(res) != 3 or any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) or int(r) < 2 for r in res):
            raise ValueError(f"resolution must be None, an int or three ints, each >= 2; got {resolution!r}")
        res = tuple(int(r) for r in res)
        if res[0] * res[1] * res[2] > MAX_GRID_POINTS:
            raise ValueError(f"a {res} grid has more than 2^31 points")
    if bounds is None:
        lo, hi = field.bounds
    else:
        try:
            lo, hi = (tuple(float(v) for v in b) for b in bounds)
        except (TypeError, ValueError):
            raise ValueError(f"bounds must be None or (lo[3], hi[3]); got {bounds!r}") from None
        with np.errstate(over="ignore"):
            ok = len(lo) == 3 and len(hi) == 3 and all(np.isfinite(np.float32(v)) for v in lo + hi) and \
                all(np.float32(h) > np.float32(l) and np.isfinite(np.float32(h) - np.float32(l)) for l, h in zip(lo, hi))
        if not ok:
            raise ValueError(f"bounds must be finite (lo[3], hi[3]) with hi > lo on every axis; got {bounds!r}")
    if direction is not None and _shape(direction, "direction") not in ((3,), (1, 3)):
        raise ValueError(f"direction must be None or one vector [3], got shape {_shape(direction, 'direction')}")
    return res, lo, hi, lattice


def _call(field, spec):
    from . import _lib
    name, _ = _storage(field)
    _check(getattr(_lib.load(), name)(_stream(field.device), C.byref(field._c), C.byref(spec)), name)


def query(field, points, directions=None, gradient=False, lanes_per_point=0):
    """field.query: see BakedField.query"""
    import torch
    from . import _lib
    from .runtime import _f32
    lead, n, mode, lanes = check_query_args(field, points, directions, lanes_per_point)
    dev = field.device
    p = _f32(points, dev).reshape(-1, 3)
    d = None
    if mode:
        d = _f32(directions, dev)
        d = d.reshape(3) if mode == 1 else torch.broadcast_to(d, p.reshape(lead + (3,)).shape).contiguous().reshape(-1, 3)
    sigma = torch.empty((n,), device=dev, dtype=torch.float32)
    rgb = torch.empty((n, 3), device=dev, dtype=torch.float32)
    grad = torch.empty((n, 3), device=dev, dtype=torch.float32) if gradient else None
    if n:
        spec = _lib.KnerfBakedQuerySpec(p.data_ptr(), n, None, None, None, None if d is None else d.data_ptr(), 1 if mode == 3 else 0,
                                        lanes << _lib.BAKED_LANES_SHIFT, sigma.data_ptr(), rgb.data_ptr(),
                                        None if grad is None else grad.data_ptr())
        _call(field, spec)
    out = (rgb.reshape(lead + (3,)), sigma.reshape(lead + (1,)))
    return out + (grad.reshape(lead + (3,)),) if gradient else out


def query_sigma(field, points, gradient=False):
    """Density alone at points [..., 3]: sigma [..., 1], with gradient=True (sigma, grad [..., 3]).  The kernels' sigma-only path: it
    loads the first word of each corner record and gives the sigma and gradient bits of query()."""
    import torch
    from . import _lib
    from .runtime import _f32
    lead, n, _, _ = check_query_args(field, points)
    dev = field.device
    p = _f32(points, dev).reshape(-1, 3)
    sigma = torch.empty((n,), device=dev, dtype=torch.float32)
    grad = torch.empty((n, 3), device=dev, dtype=torch.float32) if gradient else None
    if n:
        _call(field, _lib.KnerfBakedQuerySpec(p.data_ptr(), n, None, None, None, None, 0, 0, sigma.data_ptr(), None,
                                              None if grad is None else grad.data_ptr()))
    return (sigma.reshape(lead + (1,)), grad.reshape(lead + (3,))) if gradient else sigma.reshape(lead + (1,))


def query_grid(field, resolution, lo, hi, direction=None, sigma=True, gradient=False, lanes_per_point=0):
    """The kernels' grid mode: the field on the grid lo + idx * (hi - lo) / (R - 1) (C order, z fastest), whose points the kernel forms
    itself -> (sigma [Rx,Ry,Rz] | None, rgb [Rx,Ry,Rz,3] | None (with a direction), gradient [Rx,Ry,Rz,3] | None)"""
    import torch
    from . import _lib
    from .runtime import _f32
    lanes = check_lanes(field, lanes_per_point)
    res, lo, hi, _ = check_grid_args(field, resolution, (lo, hi), direction)
    if not sigma and direction is None and not gradient:
        raise ValueError("nothing to compute: no sigma, no direction (rgb) and no gradient")
    dev = field.device
    d = None if direction is None else _f32(direction, dev).reshape(3)
    e = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
    sig, rgb, grad = e(*res) if sigma else None, e(*res, 3) if d is not None else None, e(*res, 3) if gradient else None
    ptr = lambda t: None if t is None else t.data_ptr()
    spec = _lib.KnerfBakedQuerySpec(None, 0, (C.c_int32 * 3)(*res), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), ptr(d), 0,
                                    lanes << _lib.BAKED_LANES_SHIFT, ptr(sig), ptr(rgb), ptr(grad))
    _call(field, spec)
    return sig, rgb, grad


def stored_sigma(field):
    """The stored sigma column as a lattice, fp32 [Rx,Ry,Rz] on the device, bit for bit.  Dense: field.sigma.  Bricks (8-bit ones
    included: their records start with the same fp32 sigma): the stored bricks' first words scattered into a zeroed lattice, slab by
    slab; the record table of the dense lattice is never formed."""
    import torch
    if isinstance(field, BakedField):
        return field.sigma
    res, b = field.resolution, field.brick
    out = torch.zeros((res[0] * res[1] * res[2],), device=field.device, dtype=torch.float32)
    for s0, keys in _brick_slabs(field._brick_of, b, 4):
        lin, inside = _brick_points_device(keys, res, b)
        sig = field._records[s0:s0 + keys.numel(), :, :4].contiguous().view(torch.float32).reshape(-1)
        out[lin[inside]] = sig[inside]
    return out.reshape(res)


def density_grid(field, resolution=None, bounds=None, direction=None):
    """field.density_grid: see BakedField.density_grid"""
    res, lo, hi, lattice = check_grid_args(field, resolution, bounds, direction)
    if lattice:
        sigma = stored_sigma(field)
        return sigma if direction is None else (sigma, query_grid(field, res, lo, hi, direction, sigma=False)[1])
    sigma, rgb, _ = query_grid(field, res, lo, hi, direction)
    return sigma if direction is None else (sigma, rgb)


def extract_mesh(field, threshold, resolution=None, bounds=None, vertex_colors=False):
    """field.extract_mesh: see BakedField.extract_mesh"""
    from .runtime import marching_cubes
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not np.isfinite(threshold):
        raise ValueError(f"threshold must be a finite number, got {threshold!r}")
    _, lo, hi, _ = check_grid_args(field, resolution, bounds)
    verts, faces, normals = marching_cubes(density_grid(field, resolution, bounds), float(threshold), lo, hi)
    if not vertex_colors:
        return verts, faces, normals
    return verts, faces, normals, query(field, verts, -normals)[0]
