"""The baked field: a trained NeRF stored as a voxel grid with spherical-harmonic colour and rendered without the MLP (extension,
no reference counterpart; PlenOctrees, SNeRG and Plenoxels bake a trained NeRF in this way).

The arithmetic is HIP (csrc/baked.hip: knerf_baked_project, knerf_baked_pack, knerf_baked_render; include/knerf.h holds the contract;
BakedField.optimizer and baked_train.py: optimising the records against ray batches, csrc/baked_train.hip;
BakedField.resample and the optimiser's TV regulariser: csrc/baked_grow.hip;
BrickBakedField, the same field stored as sparse bricks behind an index table, and its renderer: csrc/baked.hip;
baked_quant.py QuantizedBrickField, the brick field with 8-bit SH coefficients, its codec and renderer: csrc/baked_quant.hip;
query, density_grid and extract_mesh of all three storages, baked_query.py: csrc/baked_query.hip);
torch is used for device memory, streams and the index plumbing of the bake only.  Host-side pieces (basis, fit matrix, record
layout) are NumPy and need no device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

MAX_DEGREE = 3
MAX_RECORD_BYTES = 1 << 40
OUTPUTS = ("image", "depth", "opacity")
SLAB_BYTES = 1 << 30       # working memory of one slab of a bake (accumulator + compensation) or of from_arrays (fp32 coefficients)
LANES = {0: (1,), 1: (1, 2), 2: (1, 4), 3: (1, 4)}        # lanes per ray the render kernel is built for, per degree


def check_degree(sh_degree) -> int:
    if isinstance(sh_degree, bool) or not isinstance(sh_degree, (int, np.integer)) or not 0 <= int(sh_degree) <= MAX_DEGREE:
        raise ValueError(f"sh_degree must be an integer 0..{MAX_DEGREE}, got {sh_degree!r}")
    return int(sh_degree)


def n_coefficients(sh_degree: int) -> int:
    return (check_degree(sh_degree) + 1) ** 2


def record_bytes(sh_degree: int) -> int:
    """fp32 sigma + 3 K halfs, padded to a multiple of 16 bytes: 16 / 32 / 64 / 112"""
    return (4 + 6 * n_coefficients(sh_degree) + 15) // 16 * 16


def sh_basis(directions, sh_degree: int) -> np.ndarray:
    """The orthonormal real spherical harmonics Y_k, k = l (l + 1) + m, without the Condon-Shortley phase, at unit vectors [..., 3]:
    [..., K] in float64 (the constants of csrc/baked.hip sh_eval)."""
    deg = check_degree(sh_degree)
    v = np.asarray(directions, dtype=np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    pi = np.pi
    Y = [np.full(x.shape, 0.5 / np.sqrt(pi))]
    if deg >= 1:
        c = np.sqrt(3.0 / (4.0 * pi))
        Y += [c * y, c * z, c * x]
    if deg >= 2:
        a, b = 0.5 * np.sqrt(15.0 / pi), 0.25 * np.sqrt(5.0 / pi)
        Y += [a * x * y, a * y * z, b * (3.0 * z * z - 1.0), a * x * z, 0.5 * a * (x * x - y * y)]
    if deg >= 3:
        a, b = 0.25 * np.sqrt(35.0 / (2.0 * pi)), 0.5 * np.sqrt(105.0 / pi)
        c, d = 0.25 * np.sqrt(21.0 / (2.0 * pi)), 0.25 * np.sqrt(7.0 / pi)
        Y += [a * y * (3.0 * x * x - y * y), b * x * y * z, c * y * (5.0 * z * z - 1.0), d * z * (5.0 * z * z - 3.0),
              c * x * (5.0 * z * z - 1.0), 0.5 * b * z * (x * x - y * y), a * x * (x * x - 3.0 * y * y)]
    return np.stack(Y, axis=-1)


def fibonacci_sphere(n: int) -> np.ndarray:
    """n unit vectors [n, 3] (float64) on the golden-angle spiral: z_i = 1 - (2 i + 1) / n, longitude i * pi (3 - sqrt 5)"""
    i = np.arange(int(n), dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / float(n)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)


def default_directions(sh_degree: int) -> int:
    K = n_coefficients(sh_degree)
    return 1 if K == 1 else max(4 * K, 16)


def fit_directions(sh_degree: int, n_directions=None):
    """(directions [D,3] float64, P = pinv(Y) [K,D] float64) of the least-squares SH fit.  Degree 0: one zero direction (the network
    seen as query(points, None) sees it) and P = 1 / Y_0.  Otherwise a Fibonacci sphere of D = n_directions (default max(4 K, 16))
    unit vectors; D < 2 K is refused."""
    K = n_coefficients(sh_degree)
    if K == 1:
        if n_directions not in (None, 1):
            raise ValueError(f"sh_degree 0 is baked from the single zero direction; n_directions must be None or 1, got {n_directions!r}")
        return np.zeros((1, 3)), np.array([[2.0 * np.sqrt(np.pi)]])
    D = default_directions(sh_degree) if n_directions is None else n_directions
    if isinstance(D, bool) or not isinstance(D, (int, np.integer)) or D < 2 * K:
        raise ValueError(f"n_directions must be an integer >= 2 K = {2 * K} for sh_degree {sh_degree}, got {n_directions!r}")
    dirs = fibonacci_sphere(int(D))
    return dirs, np.linalg.pinv(sh_basis(dirs, sh_degree))


def pack_records(sigma: np.ndarray, coefficients: np.ndarray) -> np.ndarray:
    """NumPy mirror of the record layout (knerf_baked_pack): sigma [...] fp32, coefficients [..., K, 3] fp16 -> uint8 [P, record bytes]"""
    co = np.ascontiguousarray(coefficients, dtype=np.float16)
    K = co.shape[-2]
    deg = int(round(np.sqrt(K))) - 1
    if co.shape[-1] != 3 or (deg + 1) ** 2 != K:
        raise ValueError(f"coefficients must be [..., K, 3] with K = 1, 4, 9 or 16, got {co.shape}")
    sg = np.ascontiguousarray(sigma, dtype=np.float32).reshape(-1)
    co = co.reshape(-1, 3 * K)
    if co.shape[0] != sg.size:
        raise ValueError(f"{sg.size} sigma values for {co.shape[0]} coefficient sets")
    rec = np.zeros((sg.size, record_bytes(deg)), dtype=np.uint8)
    rec[:, :4] = sg.view(np.uint8).reshape(-1, 4)
    rec[:, 4:4 + 6 * K] = co.view(np.uint8).reshape(-1, 6 * K)
    return rec


def unpack_records(records: np.ndarray, sh_degree: int):
    """the inverse of pack_records: (sigma [P] fp32, coefficients [P, K, 3] fp16)"""
    K = n_coefficients(sh_degree)
    rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, record_bytes(sh_degree))
    sg = np.ascontiguousarray(rec[:, :4]).view(np.float32).reshape(-1)
    co = np.ascontiguousarray(rec[:, 4:4 + 6 * K]).view(np.float16).reshape(-1, K, 3)
    return sg, co


BRICKS = (4, 8)            # lattice points per brick edge a BrickBakedField can have
DEFAULT_BRICK = 8


def check_brick(brick) -> int:
    if isinstance(brick, bool) or not isinstance(brick, (int, np.integer)) or int(brick) not in BRICKS:
        raise ValueError(f"brick must be one of {BRICKS} lattice points per edge, got {brick!r}")
    return int(brick)


def brick_grid(resolution, brick: int):
    """the brick grid of a lattice: ceil(R / b) bricks per axis"""
    return tuple((int(r) + brick - 1) // brick for r in resolution)


def brick_table(occupied, resolution, brick=DEFAULT_BRICK):
    """NumPy mirror of the brick table (include/knerf.h knerf_baked_bricks): occupied bool [Rx-1,Ry-1,Rz-1] -> (brick_of int32
    [Bx,By,Bz], n_bricks).  A brick is stored iff it holds a touched point (a corner of an occupied cell); stored bricks are numbered
    in ascending C order; -1 marks an absent one.  n_bricks >= 1: without an occupied cell brick 0 exists and no entry names it."""
    b = check_brick(brick)
    res = tuple(int(r) for r in resolution)
    occ = np.asarray(occupied, dtype=bool)
    if occ.shape != tuple(r - 1 for r in res):
        raise ValueError(f"occupied must be {tuple(r - 1 for r in res)} cells for a {res} lattice, got {occ.shape}")
    B = brick_grid(res, b)
    touched = np.zeros(tuple(n * b for n in B), dtype=bool)
    cx, cy, cz = occ.shape
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                touched[i:i + cx, j:j + cy, k:k + cz] |= occ
    stored = touched.reshape(B[0], b, B[1], b, B[2], b).any(axis=(1, 3, 5))
    n = int(stored.sum())
    brick_of = np.full(B, -1, dtype=np.int32)
    brick_of[stored] = np.arange(n, dtype=np.int32)
    return brick_of, max(n, 1)


def _brick_points(brick_of, resolution, b):
    """for the stored bricks of a NumPy table in slot order: (lattice index [n, b^3] int64, clipped into the lattice; inside [n, b^3] bool)"""
    res = tuple(int(r) for r in resolution)
    ids = np.argwhere(np.asarray(brick_of) >= 0)                           # ascending C order = slot order
    ax = np.arange(b)
    x = (ids[:, 0, None] * b + ax)[:, :, None, None]
    y = (ids[:, 1, None] * b + ax)[:, None, :, None]
    z = (ids[:, 2, None] * b + ax)[:, None, None, :]
    inside = (x < res[0]) & (y < res[1]) & (z < res[2])
    lin = (np.minimum(x, res[0] - 1) * res[1] + np.minimum(y, res[1] - 1)) * res[2] + np.minimum(z, res[2] - 1)
    return lin.reshape(len(ids), b ** 3).astype(np.int64), inside.reshape(len(ids), b ** 3)


def bricks_from_dense(records, brick_of, n_bricks, resolution, brick=DEFAULT_BRICK):
    """NumPy mirror of BakedField.compact: dense records uint8 [P, record bytes] -> uint8 [n_bricks, b^3, record bytes]; a stored brick
    is a verbatim copy of its points' records, points outside the lattice are all-zero"""
    b = check_brick(brick)
    rec = np.asarray(records, dtype=np.uint8)
    out = np.zeros((int(n_bricks), b ** 3, rec.shape[1]), dtype=np.uint8)
    lin, inside = _brick_points(brick_of, resolution, b)
    if len(lin):
        out[:len(lin)] = np.where(inside[:, :, None], rec[lin], 0)
    return out


def dense_from_bricks(brick_records, brick_of, resolution, brick=DEFAULT_BRICK):
    """NumPy mirror of BrickBakedField.to_dense: uint8 [n_bricks, b^3, record bytes] -> dense uint8 [P, record bytes]; records of
    absent bricks are all-zero"""
    b = check_brick(brick)
    br = np.asarray(brick_records, dtype=np.uint8)
    res = tuple(int(r) for r in resolution)
    out = np.zeros((res[0] * res[1] * res[2], br.shape[2]), dtype=np.uint8)
    lin, inside = _brick_points(brick_of, res, b)
    if len(lin):
        out[lin[inside]] = br[:len(lin)][inside]
    return out


def check_table_size(n_points: int, sh_degree: int) -> int:
    """the bytes of n_points records; ValueError at 2^40 bytes and more (the kernels refuse such a table with KNERF_ERR_INVALID)"""
    nbytes = int(n_points) * record_bytes(sh_degree)
    if nbytes >= MAX_RECORD_BYTES:
        raise ValueError(f"{int(n_points)} records of {record_bytes(sh_degree)} bytes reach 2^40 bytes; lower the resolution or sh_degree")
    return nbytes


def check_lattice_spec(resolution, bounds, sh_degree):
    """validated ((Rx,Ry,Rz), lo[3], hi[3]); ValueError on a resolution outside 2..1025, hi <= lo, or 2^40 bytes of records and more"""
    res = (resolution,) * 3 if isinstance(resolution, (int, np.integer)) and not isinstance(resolution, bool) else \
        (tuple(resolution) if isinstance(resolution, (tuple, list, np.ndarray)) else ())
    if len(res) != 3 or any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 2 <= int(r) <= 1025 for r in res):
        raise ValueError(f"resolution must be an int or three ints, each 2..1025 lattice points; got {resolution!r}")
    try:
        lo, hi = ([float(v) for v in b] for b in bounds)
    except (TypeError, ValueError):
        raise ValueError(f"bounds must be (lo[3], hi[3]); got {bounds!r}") from None
    if len(lo) != 3 or len(hi) != 3 or not all(np.isfinite(np.float32(v)) for v in lo + hi) or \
            not all(np.float32(h) > np.float32(l) for l, h in zip(lo, hi)):
        raise ValueError(f"bounds must be finite (lo[3], hi[3]) with hi > lo on every axis; got {bounds!r}")
    res = tuple(int(r) for r in res)
    check_table_size(res[0] * res[1] * res[2], sh_degree)
    return res, tuple(lo), tuple(hi)


def check_threshold(sigma_threshold) -> float:
    """a finite sigma_threshold >= 0.  With a negative one, negative densities would be stored: a cell whose corners are all negative has
    no occupancy bit (the bits mean sigma > 0) yet a non-zero trilinear sigma, and skipping it would no longer be exact."""
    try:
        thr = float(sigma_threshold)
    except (TypeError, ValueError):
        raise ValueError(f"sigma_threshold must be a number, got {sigma_threshold!r}") from None
    if isinstance(sigma_threshold, bool) or not np.isfinite(thr) or thr < 0.0:
        raise ValueError(f"sigma_threshold must be finite and >= 0, got {sigma_threshold!r}")
    return thr


def refined_resolution(resolution):
    """the lattice of one refinement, 2 r - 1 points per axis (every old point reappears in BakedField.resample, a new one sits in the
    middle of every old edge); an int or three ints -> a 3-tuple.  ValueError on a resolution outside 2..1025 and past 1025 points"""
    res = (resolution,) * 3 if isinstance(resolution, (int, np.integer)) and not isinstance(resolution, bool) else \
        (tuple(resolution) if isinstance(resolution, (tuple, list, np.ndarray)) else ())
    if len(res) != 3 or any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 2 <= int(r) <= 1025 for r in res):
        raise ValueError(f"resolution must be an int or three ints, each 2..1025 lattice points; got {resolution!r}")
    out = tuple(2 * int(r) - 1 for r in res)
    if max(out) > 1025:
        raise ValueError(f"refining {tuple(int(r) for r in res)} gives {out}: more than 1025 lattice points on an axis")
    return out


def check_render_args(step, termination, outputs, sh_degree=None, lanes_per_ray=0):
    """ValueError on step <= 0, termination outside [0, 1), unknown outputs or a lane count the degree does not have"""
    if step is not None and not (np.isfinite(float(step)) and float(step) > 0.0):
        raise ValueError(f"step must be a positive number or None, got {step!r}")
    if not 0.0 <= float(termination) < 1.0:
        raise ValueError(f"termination must lie in [0, 1), got {termination!r}")
    outs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outs or any(o not in OUTPUTS for o in outs) or len(set(outs)) != len(outs):
        raise ValueError(f"outputs must be a non-empty selection of {OUTPUTS}, got {outputs!r}")
    if lanes_per_ray != 0 and (sh_degree is None or lanes_per_ray not in LANES[sh_degree]):
        raise ValueError(f"lanes_per_ray must be 0 (default) or one of {LANES.get(sh_degree)} for sh_degree {sh_degree}, got {lanes_per_ray!r}")
    return outs


def check_colour(colour, what="background"):
    """ValueError unless `colour` is three finite numbers in [0, 1]; returns them as a tuple of floats"""
    try:
        out = tuple(float(v) for v in colour)
    except (TypeError, ValueError):
        out = ()
    if isinstance(colour, str) or len(out) != 3 or not all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in out):
        raise ValueError(f"{what} must be three finite numbers in [0, 1] (r, g, b), got {colour!r}")
    return out


def compose_background(image, opacity, background):
    """clip(image + (1 - opacity) background, 0, 1): a render over the black background put over `background` ([3] or [n,3]) on the
    host side, in the arrays' own type (torch tensors or NumPy arrays).  C <= O <= 1 up to rounding, so no kernel is needed."""
    out = image + (1.0 - opacity)[..., None] * background
    return out.clamp(0.0, 1.0) if hasattr(out, "clamp") else np.clip(out, 0.0, 1.0)


def render_over(field, background, white_background, outputs, args, kwargs):
    """field.render(*args, **kwargs) over `background`, a colour (r, g, b) or an [n,3] array of them with finite values in [0, 1]:
    the black-background launch with image and opacity, then compose_background in torch.  ValueError together with
    white_background=True (the flag is the launch's own white background) and for a background of another shape or range."""
    import torch
    if white_background:
        raise ValueError("render takes background= or white_background=True, not both")
    outs = check_render_args(None, 0.0, outputs)
    want = tuple(dict.fromkeys(outs + ("image", "opacity"))) if "image" in outs else outs
    res = field.render(*args, white_background=False, outputs=want, **kwargs)
    if "image" in outs:
        n = int(res["image"].shape[0])
        if isinstance(background, torch.Tensor) or (isinstance(background, np.ndarray) and background.ndim == 2):
            bg = background.to(device=field.device, dtype=torch.float32) if isinstance(background, torch.Tensor) else \
                torch.as_tensor(np.asarray(background, dtype=np.float32)).to(field.device)
            if tuple(bg.shape) != (n, 3) or not bool(((bg >= 0) & (bg <= 1)).all()):
                raise ValueError(f"background must be [{n}, 3] with finite values in [0, 1], got shape {tuple(bg.shape)}")
        else:
            bg = torch.tensor(check_colour(background), device=field.device, dtype=torch.float32)
        res["image"] = compose_background(res["image"], res["opacity"], bg)
    return {k: v for k, v in res.items() if k in outs or k == "stats"}


def _stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check(rc, what):
    from . import _lib
    if rc != 0:
        raise ValueError(f"{what} refused its arguments (KNERF_ERR_INVALID)") if rc == _lib.KNERF_ERR_INVALID else \
            _lib.KnerfError(f"{what} failed ({rc})")


def _ray_args(field, origins, directions, near, far, step):
    """the rays of a march as the kernels take them: (o [n,3], d [n,3], n, step, (near [n] | None, near_all), (far [n] | None, far_all));
    ValueError on mismatched counts, a step that is not a positive float32, ends that are not finite, 2^23 samples per ray and more"""
    from .runtime import _f32
    dev = field.device
    o, d = _f32(origins, dev).reshape(-1, 3), _f32(directions, dev).reshape(-1, 3)
    n = o.shape[0]
    if d.shape[0] != n:
        raise ValueError(f"{n} origins for {d.shape[0]} directions")
    h = float(step) if step is not None else 0.5 * float(min(field.cell_size))
    if not np.float32(h) > 0:
        raise ValueError(f"step {h!r} is not a positive float32")
    ends = []
    for name, v in (("near", near), ("far", far)):
        if isinstance(v, (int, float, np.floating, np.integer)):
            if not np.isfinite(np.float32(v)):
                raise ValueError(f"{name} must be finite, got {v!r}")
            ends.append((None, float(v)))
        else:
            tv = _f32(v, dev).reshape(-1)
            if tv.numel() != n:
                raise ValueError(f"{name} must be a scalar or hold one value per ray ({n}), got {tv.numel()}")
            ends.append((tv, 0.0))
    (near_t, near0), (far_t, far0) = ends
    if near_t is None and far_t is None and (far0 - near0) / h >= float(1 << 23):
        raise ValueError(f"(far - near) / step = {(far0 - near0) / h:.3g} samples per ray; at most 2^23")
    return o, d, n, h, ends[0], ends[1]


def check_depth_loss(depth_loss) -> float:
    """ValueError unless depth_loss (lambda_z, the weight of mean c (Z - z*)^2) is a finite number >= 0 as a float32; returns it"""
    ok = not isinstance(depth_loss, bool) and isinstance(depth_loss, (int, float, np.floating, np.integer))
    with np.errstate(over="ignore"):                                       # (a value beyond float32 becomes inf and is refused)
        ok = ok and bool(np.isfinite(np.float32(depth_loss)))
    if not ok or float(depth_loss) < 0.0:
        raise ValueError(f"depth_loss must be a finite number >= 0, got {depth_loss!r}")
    return float(depth_loss)


def takes_depth_loss(make):
    """Gives a grid optimiser's constructor or factory the keyword depth_loss=0.0 (lambda_z, the weight of the depth term; DESIGN.md
    2.33) beside its declared ones: keyword-only, checked (ValueError) before anything else runs, and kept on the optimiser as
    `depth_loss`, which accumulate() reads.  An __init__ gets it set on `self` before it runs (a subclass's __init__ calls its parent's
    without the keyword, which leaves the value alone); a factory gets it set on the optimiser it returns.  The declared positional
    parameters stay what they were, so every caller that passes keywords by position keeps working."""
    import functools

    @functools.wraps(make)
    def wrapped(*args, depth_loss=None, **kwargs):
        value = None if depth_loss is None else check_depth_loss(depth_loss)
        if make.__name__ == "__init__":
            if value is not None:
                args[0].depth_loss = value
            return make(*args, **kwargs)
        opt = make(*args, **kwargs)
        if value is not None:
            opt.depth_loss = value
        return opt
    return wrapped


class BakedField:
    """A lattice of (sigma fp32, 3 K fp16 SH coefficients) records over a box plus the occupancy bits of its cells; render() marches
    rays through it on the GPU.  Built by NeRF.bake, BakedField.from_arrays or BakedField.load."""

    def __init__(self, records, words, resolution, bounds, sh_degree, sigma_threshold=0.0):
        self._records, self._words = records, words          # uint8 [P, record bytes], int32 [ceil(cells / 32)] on the device
        self.resolution = tuple(int(r) for r in resolution)
        self.bounds = (tuple(float(v) for v in bounds[0]), tuple(float(v) for v in bounds[1]))
        self.sh_degree = int(sh_degree)
        self.sigma_threshold = float(sigma_threshold)
        from . import _lib
        self._c = _lib.KnerfBakedField(C.c_void_p(records.data_ptr()), C.c_void_p(words.data_ptr()), (C.c_int32 * 3)(*self.resolution),
                                       self.sh_degree, (C.c_float * 3)(*self.bounds[0]), (C.c_float * 3)(*self.bounds[1]))

    # ---- construction
    @classmethod
    def _empty(cls, sigma, resolution, lo, hi, sh_degree, sigma_threshold):
        """sigma: device fp32 lattice, already thresholded.  All-zero records and the occupancy bits; _pack fills the records in."""
        import torch
        from .runtime import occupancy_words_from_grid
        records = torch.zeros((int(sigma.numel()), record_bytes(sh_degree)), device=sigma.device, dtype=torch.uint8)
        words = occupancy_words_from_grid(sigma, 0.0, 0, what="BakedField")
        return cls(records, words, resolution, (lo, hi), sh_degree, sigma_threshold)

    def _pack(self, sigma, acc, comp, index):
        """knerf_baked_pack: the records of the points `index` (int64 [n]) from acc (+ comp) fp32 [n, K, 3]; the others keep their bytes"""
        from . import _lib
        from .runtime import _ptr
        n = int(index.numel())
        if n:
            _check(_lib.load().knerf_baked_pack(_stream(sigma.device), _ptr(sigma), _ptr(acc), _ptr(comp), _ptr(index), n,
                                                int(sigma.numel()), self.sh_degree, _ptr(self._records)), "knerf_baked_pack")

    @classmethod
    def from_arrays(cls, sigma, coefficients, bounds, sigma_threshold=0.0, device=None):
        """sigma [Rx,Ry,Rz] fp32 and coefficients [Rx,Ry,Rz,K,3] fp16 / fp32 (NumPy or torch) over bounds = (lo[3], hi[3]): packs the
        records on the device, stores every sigma <= sigma_threshold as 0 and builds the occupancy bits.  sigma_threshold >= 0: no
        negative density is stored, so a cell without an occupancy bit has sigma = 0 at all 8 corners."""
        import torch
        co = coefficients if isinstance(coefficients, torch.Tensor) else torch.as_tensor(np.asarray(coefficients))
        sg = sigma if isinstance(sigma, torch.Tensor) else torch.as_tensor(np.asarray(sigma, dtype=np.float32))
        if sg.dim() != 3 or co.dim() != 5 or tuple(co.shape[:3]) != tuple(sg.shape) or co.shape[4] != 3 or \
                co.shape[3] not in (1, 4, 9, 16):
            raise ValueError(f"need sigma [Rx,Ry,Rz] and coefficients [Rx,Ry,Rz,K,3] with K = 1, 4, 9 or 16; got {tuple(sg.shape)} and "
                             f"{tuple(co.shape)}")
        if co.dtype not in (torch.float16, torch.float32):
            raise ValueError(f"coefficients must be float16 or float32, got {co.dtype}")
        deg = int(round(np.sqrt(co.shape[3]))) - 1
        res, lo, hi = check_lattice_spec(tuple(sg.shape), bounds, deg)
        thr = check_threshold(sigma_threshold)
        dev = torch.device(device if device is not None else (sg.device if sg.is_cuda else "cuda"))
        sg = sg.to(device=dev, dtype=torch.float32).contiguous()
        sg = torch.where(sg > thr, sg, torch.zeros_like(sg))
        field = cls._empty(sg, res, lo, hi, deg, thr)
        K = co.shape[3]
        co = co.reshape(-1, K, 3)
        slab = max(1, SLAB_BYTES // (12 * K))                 # the fp32 copy of a slab's coefficients stays under about 1 GB
        for s0 in range(0, co.shape[0], slab):
            acc = co[s0:s0 + slab].to(device=dev, dtype=torch.float32).contiguous()
            field._pack(sg, acc, None, torch.arange(s0, s0 + acc.shape[0], device=dev, dtype=torch.int64))
        return field

    @classmethod
    def uniform(cls, resolution, bounds, sh_degree, sigma=0.1, colour=0.5, device=None):
        """A field with the same record at every lattice point, built on the device: density `sigma` (finite, >= 0) and the grey
        `colour` in every direction (the DC coefficient is colour 2 sqrt(pi) = colour / Y_0, all other coefficients are 0): what a
        grid trainer starts from when there is no MLP to bake (baked_train.fit_coarse_to_fine).  sigma_threshold is 0."""
        import torch
        from .runtime import occupancy_words_from_grid
        deg = check_degree(sh_degree)
        res, lo, hi = check_lattice_spec(resolution, bounds, deg)
        for name, v in (("sigma", sigma), ("colour", colour)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(np.float32(v)):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        if float(sigma) < 0.0:
            raise ValueError(f"sigma must be >= 0, got {sigma!r}")
        with np.errstate(over="ignore"):
            dc = np.float16(float(colour) * 2.0 * np.sqrt(np.pi))
        if not np.isfinite(dc):
            raise ValueError(f"colour {colour!r} gives a DC coefficient that is no finite float16")
        K = n_coefficients(deg)
        co = np.zeros((1, K, 3), dtype=np.float16)
        co[0, 0, :] = dc
        one = pack_records(np.full((1,), sigma, dtype=np.float32), co)
        dev = torch.device(device if device is not None else "cuda")
        n = res[0] * res[1] * res[2]
        records = torch.as_tensor(one).to(dev).repeat(n, 1).contiguous()
        words = occupancy_words_from_grid(torch.full(res, float(np.float32(sigma)), device=dev, dtype=torch.float32), 0.0, 0,
                                          what="BakedField.uniform")
        return cls(records, words, res, (lo, hi), deg, 0.0)

    def resample(self, resolution, sigma_threshold=None):
        """This field on another lattice (an int or three ints, 2..1025 points per axis) over the same box: knerf_baked_resample
        (trilinear, specified in include/knerf.h), every new sigma <= sigma_threshold (default: the field's own) stored as 0 and the
        occupancy bits rebuilt from the new sigma.  A cell that was empty stays empty, so skipping stays exact; with
        refined_resolution(self.resolution) every old lattice point keeps its values.  This field is left as it is."""
        import torch
        from . import _lib
        from .runtime import _ptr, occupancy_words_from_grid
        res, _, _ = check_lattice_spec(resolution, self.bounds, self.sh_degree)
        thr = self.sigma_threshold if sigma_threshold is None else check_threshold(sigma_threshold)
        dev = self.device
        records = torch.empty((res[0] * res[1] * res[2], record_bytes(self.sh_degree)), device=dev, dtype=torch.uint8)
        _check(_lib.load().knerf_baked_resample(_stream(dev), C.byref(self._c), (C.c_int32 * 3)(*res), thr, _ptr(records)),
               "knerf_baked_resample")
        sigma = records[:, :4].contiguous().view(torch.float32).reshape(res)
        words = occupancy_words_from_grid(sigma, 0.0, 0, what="BakedField.resample")
        return BakedField(records, words, res, self.bounds, self.sh_degree, thr)

    # ---- the unpacked views
    @property
    def device(self):
        return self._records.device

    @property
    def sigma(self):
        """fp32 [Rx,Ry,Rz] (a copy out of the records)"""
        import torch
        return self._records[:, :4].contiguous().view(torch.float32).reshape(self.resolution)

    @property
    def coefficients(self):
        """fp16 [Rx,Ry,Rz,K,3] (a copy out of the records)"""
        import torch
        K = n_coefficients(self.sh_degree)
        return self._records[:, 4:4 + 6 * K].contiguous().view(torch.float16).reshape(self.resolution + (K, 3))

    @property
    def occupied(self):
        """bool [Rx-1,Ry-1,Rz-1] on the device: the cells with sigma > 0 at one of their corners"""
        return _unpack_words(self._words, tuple(r - 1 for r in self.resolution))

    @property
    def cell_size(self):
        return tuple((np.float32(h) - np.float32(l)) / (r - 1) for l, h, r in zip(self.bounds[0], self.bounds[1], self.resolution))

    # ---- persistence
    KEYS = ("format", "records", "words", "resolution", "lo", "hi", "sh_degree", "sigma_threshold")

    def save(self, path):
        """one .npz file at exactly `path` (no suffix is appended): the records and bits as they are on the device, resolution,
        bounds, degree, threshold"""
        with open(path, "wb") as f:
            np.savez(f, records=self._records.cpu().numpy(), words=self._words.cpu().numpy(),
                     resolution=np.asarray(self.resolution, dtype=np.int32), lo=np.asarray(self.bounds[0], dtype=np.float64),
                     hi=np.asarray(self.bounds[1], dtype=np.float64), sh_degree=np.int32(self.sh_degree),
                     sigma_threshold=np.float64(self.sigma_threshold), format=np.int32(1))

    @classmethod
    def load(cls, path, device=None):
        """the field save(path) wrote; ValueError on a file that is not one.  The padding of the records is never read as data."""
        import torch
        with np.load(path) as z:
            missing = [k for k in cls.KEYS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a baked field (missing {missing})")
            if int(z["format"]) != 1:
                raise ValueError(f"{path}: unknown baked-field format {int(z['format'])}")
            deg = check_degree(int(z["sh_degree"]))
            res, lo, hi = check_lattice_spec(tuple(int(r) for r in z["resolution"]), (z["lo"], z["hi"]), deg)
            records, words = z["records"], z["words"]
            n_points, cells = int(np.prod(res)), int(np.prod([r - 1 for r in res]))
            if records.dtype != np.uint8 or records.shape != (n_points, record_bytes(deg)) or words.dtype != np.int32 or \
                    words.shape != ((cells + 31) // 32,):
                raise ValueError(f"{path}: records {records.shape} / bits {words.shape} do not fit a {res} lattice of degree {deg}")
            dev = torch.device(device if device is not None else "cuda")
            return cls(torch.as_tensor(records).to(dev), torch.as_tensor(words).to(dev), res, (lo, hi), deg, float(z["sigma_threshold"]))

    # ---- rendering
    def render(self, origins, directions, near, far, step=None, white_background=False, termination=0.0,
               outputs=("image", "depth", "opacity"), skip_empty=True, stats=False, lanes_per_ray=0, background=None):
        """Volume rendering of rays (origins, directions [N,3]; directions need not be unit vectors, t is in units of |d|) between
        near and far (scalars or [N]) with samples every `step` (None: half the smallest cell edge): {"image": [N,3], "depth": [N],
        "opacity": [N]} restricted to `outputs`, and with stats=True also "stats": int64 [2] device tensor (samples fetched, samples
        inside [near, far] of all rays).  The march is specified in include/knerf.h (knerf_baked_render).  skip_empty only saves
        work: the outputs are bit-identical without it.  lanes_per_ray is a tuning / diagnostic knob for tests and tools/baked_bench.py,
        not a promised part of the interface: it picks the kernel variant (0, the default: the library's choice; the variants differ
        in summation order only).  background: a colour (r, g, b) or an [N,3] tensor of them, values in [0, 1]: the image is
        clip(image + (1 - opacity) background, 0, 1), composed in torch from the black-background launch (render_over; every other
        output is that launch's); not together with white_background=True."""
        if background is not None:
            return render_over(self, background, white_background, outputs, (origins, directions, near, far),
                               dict(step=step, termination=termination, skip_empty=skip_empty, stats=stats, lanes_per_ray=lanes_per_ray))
        import torch
        from . import _lib
        from .runtime import _ptr
        outs = check_render_args(step, termination, outputs, self.sh_degree, lanes_per_ray)
        dev = self.device
        o, d, n, h, (near_t, near0), (far_t, far0) = _ray_args(self, origins, directions, near, far, step)
        e = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
        res = {"image": e(n, 3) if "image" in outs else None, "depth": e(n) if "depth" in outs else None,
               "opacity": e(n) if "opacity" in outs else None}
        counter = torch.zeros(2, device=dev, dtype=torch.int64) if stats else None
        flags = (_lib.BAKED_WHITE_BACKGROUND if white_background else 0) | (_lib.BAKED_SKIP_EMPTY if skip_empty else 0) | \
            (int(lanes_per_ray) << _lib.BAKED_LANES_SHIFT)
        if n:
            _check(_lib.load().knerf_baked_render(_stream(dev), C.byref(self._c), _ptr(o), _ptr(d), _ptr(near_t), _ptr(far_t), near0, far0, n,
                                                  h, float(termination), flags, _ptr(res["image"]), _ptr(res["depth"]),
                                                  _ptr(res["opacity"]), _ptr(counter)), "knerf_baked_render")
        out = {k: v for k, v in res.items() if v is not None}
        if stats:
            out["stats"] = counter
        return out

    # ---- optimisation against ray batches
    @takes_depth_loss
    def optimizer(self, learning_rate_sigma, learning_rate_sh, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dilation=0, step=None,
                  white_background=False, termination=0.0, lanes_per_ray=0, tv_sigma=0.0, tv_sh=0.0, tv_epsilon=1e-6, loss=None,
                  regularizers=None, background=None, opacity_loss=0.0, target_background=None, background_seed=0):
        """A BakedFieldOptimizer (baked_train.py) over a COPY of this field's records: Adam on sigma and the SH coefficients of the
        lattice points around the occupied cells (grown by `dilation` cells) against batches of rays and their colours; this field
        itself is left as it is.  step, white_background, termination, lanes_per_ray: how the optimiser marches, as in render().
        tv_sigma, tv_sh (>= 0, default off): the weights of the total-variation regulariser on density and on the colour coefficients
        (knerf_baked_train_tv; each is the weight of the MEAN term over the slots, resp. over the slots and the 3 K coefficient
        columns), tv_epsilon (> 0) the constant under its root.  With both weights 0 a step is what it is without them.
        loss, regularizers: the objective, as NeRF.compile takes it (a name, a keras_nerf_amd.losses class, a Keras loss object or its
        serialised dict; losses.RayRegularizers(distortion=, opacity_entropy=) with the default nets): knerf_baked_train_rays_ext.
        Default, and "mse" without a regulariser: the mean squared error, the launches and bits of an optimiser without them.
        background (None | "black" | "white" | "random" | (r, g, b)), opacity_loss (>= 0), target_background (None | "black" | "white":
        what the targets' rgb is composited over; default: the white flag), background_seed: training on RGBA targets [n,4]
        (knerf_baked_train_rays_rgba).  "white" equals white_background=True; "random" draws torch.rand((n, 3)) per
        launch from a generator seeded once; opacity_loss weighs the mean of (O - alpha)^2.  "random" and opacity_loss > 0 need
        [n,4] targets.  Without these keywords the optimiser makes exactly the calls it made before them.
        depth_loss (>= 0, default off): the weight of the mean over the rays of c (Z - z*)^2 between a ray's expected depth Z (what
        render() writes as depth) and a depth target z* per ray with weight c, given to accumulate() / train_step() as depth= and
        depth_weight= (knerf_baked_train_rays_depth).  With 0 the optimiser makes exactly the calls it made before."""
        from .baked_train import BakedFieldOptimizer
        return BakedFieldOptimizer(self, learning_rate_sigma=learning_rate_sigma, learning_rate_sh=learning_rate_sh, beta_1=beta_1,
                                   beta_2=beta_2, epsilon=epsilon, dilation=dilation, step=step, white_background=white_background,
                                   termination=termination, lanes_per_ray=lanes_per_ray, tv_sigma=tv_sigma, tv_sh=tv_sh,
                                   tv_epsilon=tv_epsilon, loss=loss, regularizers=regularizers, background=background,
                                   opacity_loss=opacity_loss, target_background=target_background, background_seed=background_seed)

    # ---- how the objective moves when a ray moves (baked_pose.py: refining camera poses)
    def ray_gradients(self, origins, directions, near, far, target, step=None, white_background=False, termination=0.0, n_total=None,
                      lanes_per_ray=0):
        """baked_pose.ray_gradients(self, ...): (grad_origin [N,3], grad_direction [N,3], loss) of the squared error against `target`"""
        from .baked_pose import ray_gradients
        return ray_gradients(self, origins, directions, near, far, target, step=step, white_background=white_background,
                             termination=termination, n_total=n_total, lanes_per_ray=lanes_per_ray)

    # ---- the field at points, on grids and as a mesh (baked_query.py)
    def query(self, points, directions=None, gradient=False, lanes_per_point=0):
        """What the field holds at points [..., 3] (any leading shape), seen along directions None, [3] or [..., 3] (shapes and
        broadcasting as NeRF.query): (rgb [..., 3], sigma [..., 1]) and with gradient=True also grad [..., 3], the exact gradient of
        the trilinear sigma inside the point's cell; torch tensors on the field's device.  It is the renderer's evaluation of one
        sample (include/knerf.h knerf_baked_query): outside the box everything is 0; no direction, or one of length 0, gives the DC
        colour.  lanes_per_point picks the kernel variant as render's lanes_per_ray does."""
        from .baked_query import query
        return query(self, points, directions, gradient, lanes_per_point)

    def density_grid(self, resolution=None, bounds=None, direction=None):
        """NeRF.density_grid on this field: sigma [Rx,Ry,Rz] on the grid lo + idx (hi - lo) / (R - 1), or (sigma, rgb [Rx,Ry,Rz,3]) with a
        direction [3].  bounds=None: the field's own box; resolution=None: the field's own resolution.  With neither, the grid is the
        lattice itself and sigma is the stored sigma column, bit for bit (no coordinate arithmetic)."""
        from .baked_query import density_grid
        return density_grid(self, resolution, bounds, direction)

    def extract_mesh(self, threshold, resolution=None, bounds=None, vertex_colors=False):
        """runtime.marching_cubes(self.density_grid(resolution, bounds), threshold, lo, hi): (vertices [V,3], faces [F,3] int32, normals
        [V,3]); vertex_colors: also self.query(vertices, -normals)[0], the convention of NeRF.extract_mesh.  An empty surface gives
        empty arrays.  keras_nerf_amd.io.ply.save_ply writes the result."""
        from .baked_query import extract_mesh
        return extract_mesh(self, threshold, resolution, bounds, vertex_colors)

    # ---- sparse storage
    def compact(self, brick=DEFAULT_BRICK):
        """This field as a BrickBakedField: only the bricks of brick^3 lattice points (4 or 8) that hold a corner of an occupied cell
        are kept, behind an index table (include/knerf.h knerf_baked_bricks).  It renders the same bits.  This field is left as it is."""
        import torch
        b = check_brick(brick)
        brick_of, n = _brick_table_device(self.occupied, self.resolution, b)
        check_table_size(max(n, 1) * b ** 3, self.sh_degree)
        records = torch.zeros((max(n, 1), b ** 3, record_bytes(self.sh_degree)), device=self.device, dtype=torch.uint8)
        _gather_bricks(self._records.view(torch.int32), brick_of, self.resolution, b, records.view(torch.int32))
        return BrickBakedField(records, brick_of, self._words, self.resolution, self.bounds, self.sh_degree, b, self.sigma_threshold)

    def quantize(self, brick=DEFAULT_BRICK, bits=8):
        """compact(brick).quantize(bits): this field as a baked_quant.QuantizedBrickField"""
        return self.compact(brick).quantize(bits)


def _brick_table_device(occupied, resolution, b):
    """brick_table on the device: occupied bool [Rx-1,Ry-1,Rz-1] -> (brick_of int32 [Bx,By,Bz], number of stored bricks; the one host
    read)"""
    import torch
    B = brick_grid(resolution, b)
    touched = torch.zeros(tuple(n * b for n in B), device=occupied.device, dtype=torch.bool)
    cx, cy, cz = occupied.shape
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                touched[i:i + cx, j:j + cy, k:k + cz] |= occupied
    stored = touched.reshape(B[0], b, B[1], b, B[2], b).any(dim=5).any(dim=3).any(dim=1)
    slot = torch.cumsum(stored.reshape(-1).to(torch.int32), 0, dtype=torch.int32).reshape(B) - 1
    return torch.where(stored, slot, torch.full_like(slot, -1)).contiguous(), int(stored.sum())


def _brick_points_device(keys, resolution, b):
    """the lattice points of the bricks `keys` (int64 [m], linear brick indices): (lattice index int64 [m b^3], clipped into the
    lattice; inside bool [m b^3])"""
    import torch
    res, B = resolution, brick_grid(resolution, b)
    ax = torch.arange(b, device=keys.device, dtype=torch.int64)
    x = ((keys // (B[1] * B[2])) * b)[:, None] + ax
    y = (((keys // B[2]) % B[1]) * b)[:, None] + ax
    z = ((keys % B[2]) * b)[:, None] + ax
    x, y, z = x[:, :, None, None], y[:, None, :, None], z[:, None, None, :]
    inside = (x < res[0]) & (y < res[1]) & (z < res[2])
    lin = (x.clamp(max=res[0] - 1) * res[1] + y.clamp(max=res[1] - 1)) * res[2] + z.clamp(max=res[2] - 1)
    return lin.reshape(-1), inside.reshape(-1)


def _brick_slabs(brick_of, b, row_bytes):
    """the stored bricks' linear indices (ascending = slot order) in slabs whose rows and index plumbing stay under SLAB_BYTES"""
    keys = (brick_of.reshape(-1) >= 0).nonzero().reshape(-1)
    per = max(1, SLAB_BYTES // (b ** 3 * (row_bytes + 24)))
    return [(s0, keys[s0:s0 + per]) for s0 in range(0, int(keys.numel()), per)]


def _gather_bricks(table, brick_of, resolution, b, out):
    """out[slot][place] = table[point] for every point of every stored brick, zeros outside the lattice; table [P, w], out
    [n_bricks, b^3, w].  Slab by slab: no second copy of the table is held."""
    for s0, keys in _brick_slabs(brick_of, b, table.shape[1] * table.element_size()):
        lin, inside = _brick_points_device(keys, resolution, b)
        rows = table[lin]
        rows[~inside] = 0
        out[s0:s0 + keys.numel()] = rows.reshape(keys.numel(), b ** 3, -1)


BRICK_KEYS = ("format", "records", "brick_of", "words", "brick", "resolution", "lo", "hi", "sh_degree", "sigma_threshold")


def read_brick_file(path) -> dict:
    """The arrays of a file BrickBakedField.save wrote (format 2), validated on the host: {"records" uint8 [n_bricks, b^3, record
    bytes], "brick_of" int32 [Bx,By,Bz], "words" int32, "brick", "n_bricks", "resolution", "lo", "hi", "sh_degree",
    "sigma_threshold"}.  ValueError on a missing key, another format, a shape or dtype that does not fit, and a brick table whose
    entries >= 0 are not exactly 0..n_bricks-1 in ascending order (an entry past the records, a repeated slot, slots out of order).
    No device is touched."""
    with np.load(path) as z:
        missing = [k for k in BRICK_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a brick baked field (missing {missing})")
        if np.ndim(z["format"]) != 0 or int(z["format"]) != 2:
            raise ValueError(f"{path}: baked-field format {z['format']!r} is not the brick format 2")
        data = {k: z[k] for k in BRICK_KEYS}
    for k in ("sh_degree", "brick", "sigma_threshold"):
        if np.ndim(data[k]) != 0:
            raise ValueError(f"{path}: {k} must be a scalar, got shape {np.shape(data[k])}")
    for k in ("resolution", "lo", "hi"):
        if np.shape(data[k]) != (3,):
            raise ValueError(f"{path}: {k} must hold three values, got shape {np.shape(data[k])}")
    if data["sh_degree"].dtype.kind not in "iu" or data["brick"].dtype.kind not in "iu" or data["resolution"].dtype.kind not in "iu":
        raise ValueError(f"{path}: sh_degree, brick and resolution must be integers")
    deg = check_degree(int(data["sh_degree"]))
    b = check_brick(int(data["brick"]))
    res, lo, hi = check_lattice_spec(tuple(int(r) for r in data["resolution"]), (data["lo"], data["hi"]), deg)
    thr = check_threshold(float(data["sigma_threshold"]))
    brick_of, records, words = data["brick_of"], data["records"], data["words"]
    B = brick_grid(res, b)
    if brick_of.dtype != np.int32 or brick_of.shape != B:
        raise ValueError(f"{path}: brick table {brick_of.dtype} {brick_of.shape} does not fit the {B} bricks of a {res} lattice")
    slots = brick_of.reshape(-1)[brick_of.reshape(-1) >= 0]
    if (brick_of < -1).any() or not np.array_equal(slots, np.arange(slots.size, dtype=np.int32)):
        raise ValueError(f"{path}: the brick table's slots are not 0..n-1 in ascending order (out of range, repeated or out of order)")
    n_bricks = max(int(slots.size), 1)
    cells = int(np.prod([r - 1 for r in res]))
    if records.dtype != np.uint8 or records.shape != (n_bricks, b ** 3, record_bytes(deg)) or words.dtype != np.int32 or \
            words.shape != ((cells + 31) // 32,):
        raise ValueError(f"{path}: records {records.dtype} {records.shape} / bits {words.dtype} {words.shape} do not fit {n_bricks} "
                         f"bricks of {b}^3 records of degree {deg} on a {res} lattice")
    check_table_size(n_bricks * b ** 3, deg)
    return {"records": records, "brick_of": brick_of, "words": words, "brick": b, "n_bricks": n_bricks, "resolution": res, "lo": lo,
            "hi": hi, "sh_degree": deg, "sigma_threshold": thr}


def load_field(path, device=None):
    """BakedField.load, BrickBakedField.load or QuantizedBrickField.load, whichever wrote `path` (its format says)"""
    with np.load(path) as z:
        if "format" not in z.files or np.ndim(z["format"]) != 0:
            raise ValueError(f"{path}: not a baked field (no format)")
        fmt = int(z["format"])
    if fmt == 1:
        return BakedField.load(path, device)
    if fmt == 2:
        return BrickBakedField.load(path, device)
    if fmt == 3:
        from .baked_quant import QuantizedBrickField
        return QuantizedBrickField.load(path, device)
    raise ValueError(f"{path}: unknown baked-field format {fmt}")


class BrickBakedField:
    """A BakedField stored sparsely (include/knerf.h knerf_baked_bricks): the lattice cut into bricks of brick^3 points, only those with
    a corner of an occupied cell stored, behind the int32 table brick_of [Bx,By,Bz] (slot or -1); every other record reads as zero.
    render() marches rays through it on the GPU and gives the bits of the dense field's render().  Built by BakedField.compact,
    NeRF.bake(bricks=...) or BrickBakedField.load; to_dense() leads back.  baked_train.brick_optimizer(field, ...) optimises it as it
    is; baked_bricks_grow has resampling, the total-variation regulariser, pruning and coarse-to-fine fitting on bricks."""

    def __init__(self, records, brick_of, words, resolution, bounds, sh_degree, brick=DEFAULT_BRICK, sigma_threshold=0.0):
        # uint8 [n_bricks, b^3, record bytes], int32 [Bx,By,Bz], int32 [ceil(cells / 32)] on the device
        self._records, self._brick_of, self._words = records, brick_of, words
        self.resolution = tuple(int(r) for r in resolution)
        self.bounds = (tuple(float(v) for v in bounds[0]), tuple(float(v) for v in bounds[1]))
        self.sh_degree = check_degree(sh_degree)
        self.brick = check_brick(brick)
        self.sigma_threshold = float(sigma_threshold)
        if records.dim() != 3 or tuple(records.shape[1:]) != (self.brick ** 3, record_bytes(self.sh_degree)) or records.shape[0] < 1 or \
                tuple(brick_of.shape) != brick_grid(self.resolution, self.brick):
            raise ValueError(f"records {tuple(records.shape)} / brick table {tuple(brick_of.shape)} do not fit bricks of {self.brick}^3 "
                             f"records of degree {self.sh_degree} on a {self.resolution} lattice")
        self.n_bricks = int(records.shape[0])
        from . import _lib
        self._c = _lib.KnerfBakedBricks(C.c_void_p(records.data_ptr()), C.c_void_p(brick_of.data_ptr()), C.c_void_p(words.data_ptr()),
                                        (C.c_int32 * 3)(*self.resolution), self.sh_degree, (C.c_float * 3)(*self.bounds[0]),
                                        (C.c_float * 3)(*self.bounds[1]), self.brick.bit_length() - 1, self.n_bricks)
        self._bake_sigma = None                              # fp32 [n_bricks b^3]: sigma in brick order while a bake fills the records

    # ---- construction by the baker
    @classmethod
    def _empty(cls, sigma, resolution, lo, hi, sh_degree, sigma_threshold, brick):
        """sigma: device fp32 lattice, already thresholded.  The occupancy bits, the brick table, all-zero brick records and sigma in
        brick order; _pack fills the records in."""
        import torch
        from .runtime import occupancy_words_from_grid
        words = occupancy_words_from_grid(sigma, 0.0, 0, what="BrickBakedField")
        brick_of, n = _brick_table_device(_unpack_words(words, tuple(r - 1 for r in resolution)), resolution, brick)
        check_table_size(max(n, 1) * brick ** 3, sh_degree)
        records = torch.zeros((max(n, 1), brick ** 3, record_bytes(sh_degree)), device=sigma.device, dtype=torch.uint8)
        field = cls(records, brick_of, words, resolution, (lo, hi), sh_degree, brick, sigma_threshold)
        field._bake_sigma = torch.zeros((max(n, 1), brick ** 3, 1), device=sigma.device, dtype=torch.float32)
        _gather_bricks(sigma.reshape(-1, 1), brick_of, field.resolution, brick, field._bake_sigma)
        return field

    def _pack(self, sigma, acc, comp, index):
        """BakedField._pack with the destinations in brick order: `index` (int64 [n]) names LATTICE points, all of them in stored bricks;
        knerf_baked_pack writes record slot b^3 + place of each and takes its sigma from the brick-ordered copy"""
        from . import _lib
        from .runtime import _ptr
        n = int(index.numel())
        if n:
            res, b, L = self.resolution, self.brick, self.brick.bit_length() - 1
            B = brick_grid(res, b)
            x, y, z = index // (res[1] * res[2]), (index // res[2]) % res[1], index % res[2]
            slot = self._brick_of.reshape(-1)[((x >> L) * B[1] + (y >> L)) * B[2] + (z >> L)].to(index.dtype)
            dest = ((slot * b + (x & (b - 1))) * b + (y & (b - 1))) * b + (z & (b - 1))
            _check(_lib.load().knerf_baked_pack(_stream(sigma.device), _ptr(self._bake_sigma), _ptr(acc), _ptr(comp), _ptr(dest.contiguous()), n,
                                                self.n_bricks * b ** 3, self.sh_degree, _ptr(self._records)), "knerf_baked_pack")

    @property
    def device(self):
        return self._records.device

    @property
    def brick_of(self):
        """int32 [Bx,By,Bz] on the device: the slot of every brick, -1 for an absent one"""
        return self._brick_of

    @property
    def occupied(self):
        """bool [Rx-1,Ry-1,Rz-1] on the device: the cells with sigma > 0 at one of their corners"""
        return _unpack_words(self._words, tuple(r - 1 for r in self.resolution))

    @property
    def cell_size(self):
        return tuple((np.float32(h) - np.float32(l)) / (r - 1) for l, h, r in zip(self.bounds[0], self.bounds[1], self.resolution))

    @property
    def nbytes(self):
        """bytes on the device: records + brick table + occupancy bits"""
        return sum(int(t.numel()) * t.element_size() for t in (self._records, self._brick_of, self._words))

    def to_dense(self) -> BakedField:
        """the BakedField with this field's stored bricks copied back and every other record zero"""
        import torch
        res, b = self.resolution, self.brick
        check_table_size(res[0] * res[1] * res[2], self.sh_degree)
        records = torch.zeros((res[0] * res[1] * res[2], record_bytes(self.sh_degree)), device=self.device, dtype=torch.uint8)
        dst, src = records.view(torch.int32), self._records.view(torch.int32)            # rows move as words, not as bytes
        for s0, keys in _brick_slabs(self._brick_of, b, records.shape[1]):
            lin, inside = _brick_points_device(keys, res, b)
            dst[lin[inside]] = src[s0:s0 + keys.numel()].reshape(-1, dst.shape[1])[inside]
        return BakedField(records, self._words, res, self.bounds, self.sh_degree, self.sigma_threshold)

    # ---- persistence
    def save(self, path):
        """one .npz file at exactly `path` (no suffix is appended), format 2: the brick records, the brick table and the bits as they
        are on the device, the brick edge, and resolution, bounds, degree, threshold as BakedField.save writes them"""
        with open(path, "wb") as f:
            np.savez(f, records=self._records.cpu().numpy(), brick_of=self._brick_of.cpu().numpy(), words=self._words.cpu().numpy(),
                     brick=np.int32(self.brick), resolution=np.asarray(self.resolution, dtype=np.int32),
                     lo=np.asarray(self.bounds[0], dtype=np.float64), hi=np.asarray(self.bounds[1], dtype=np.float64),
                     sh_degree=np.int32(self.sh_degree), sigma_threshold=np.float64(self.sigma_threshold), format=np.int32(2))

    @classmethod
    def load(cls, path, device=None):
        """the field save(path) wrote; ValueError on a file that is not one (read_brick_file checks it before anything is uploaded)"""
        import torch
        d = read_brick_file(path)
        dev = torch.device(device if device is not None else "cuda")
        return cls(torch.as_tensor(d["records"]).to(dev), torch.as_tensor(d["brick_of"]).to(dev), torch.as_tensor(d["words"]).to(dev),
                   d["resolution"], (d["lo"], d["hi"]), d["sh_degree"], d["brick"], d["sigma_threshold"])

    # ---- rendering
    def render(self, origins, directions, near, far, step=None, white_background=False, termination=0.0,
               outputs=("image", "depth", "opacity"), skip_empty=True, stats=False, lanes_per_ray=0, background=None):
        """BakedField.render through the brick table (knerf_baked_render_bricks): the same arguments, checks and result dict, and for
        a field that came from compact() the same bits."""
        if background is not None:      # a colour or [n,3]: the black-background launch composed on the host (render_over)
            return render_over(self, background, white_background, outputs, (origins, directions, near, far),
                               dict(step=step, termination=termination, skip_empty=skip_empty, stats=stats, lanes_per_ray=lanes_per_ray))
        import torch
        from . import _lib
        from .runtime import _ptr
        outs = check_render_args(step, termination, outputs, self.sh_degree, lanes_per_ray)
        dev = self.device
        o, d, n, h, (near_t, near0), (far_t, far0) = _ray_args(self, origins, directions, near, far, step)
        e = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
        res = {"image": e(n, 3) if "image" in outs else None, "depth": e(n) if "depth" in outs else None,
               "opacity": e(n) if "opacity" in outs else None}
        counter = torch.zeros(2, device=dev, dtype=torch.int64) if stats else None
        flags = (_lib.BAKED_WHITE_BACKGROUND if white_background else 0) | (_lib.BAKED_SKIP_EMPTY if skip_empty else 0) | \
            (int(lanes_per_ray) << _lib.BAKED_LANES_SHIFT)
        if n:
            _check(_lib.load().knerf_baked_render_bricks(_stream(dev), C.byref(self._c), _ptr(o), _ptr(d), _ptr(near_t), _ptr(far_t), near0,
                                                         far0, n, h, float(termination), flags, _ptr(res["image"]), _ptr(res["depth"]),
                                                         _ptr(res["opacity"]), _ptr(counter)), "knerf_baked_render_bricks")
        out = {k: v for k, v in res.items() if v is not None}
        if stats:
            out["stats"] = counter
        return out

    # ---- how the objective moves when a ray moves (baked_pose.py: refining camera poses)
    def ray_gradients(self, origins, directions, near, far, target, step=None, white_background=False, termination=0.0, n_total=None,
                      lanes_per_ray=0):
        """baked_pose.ray_gradients(self, ...): (grad_origin [N,3], grad_direction [N,3], loss) of the squared error against `target`"""
        from .baked_pose import ray_gradients
        return ray_gradients(self, origins, directions, near, far, target, step=step, white_background=white_background,
                             termination=termination, n_total=n_total, lanes_per_ray=lanes_per_ray)

    # ---- the field at points, on grids and as a mesh (baked_query.py): BakedField.query / density_grid / extract_mesh on this storage
    def query(self, points, directions=None, gradient=False, lanes_per_point=0):
        """BakedField.query through the brick table (knerf_baked_query_bricks): the same bits"""
        from .baked_query import query
        return query(self, points, directions, gradient, lanes_per_point)

    def density_grid(self, resolution=None, bounds=None, direction=None):
        """BakedField.density_grid; the lattice itself is scattered out of the stored bricks, the dense record table is never formed"""
        from .baked_query import density_grid
        return density_grid(self, resolution, bounds, direction)

    def extract_mesh(self, threshold, resolution=None, bounds=None, vertex_colors=False):
        """BakedField.extract_mesh"""
        from .baked_query import extract_mesh
        return extract_mesh(self, threshold, resolution, bounds, vertex_colors)

    # ---- 8-bit SH coefficients
    def quantize(self, bits=8):
        """This field as a baked_quant.QuantizedBrickField (knerf_baked_quantize_bricks; the format is stated in include/knerf.h
        knerf_baked_qbricks): the SH coefficients as 8-bit values with one power-of-two scale per brick and SH band, records of
        8 / 16 / 32 / 64 bytes; density, the brick table and the occupancy bits are shared with this field, which is left as it is.
        bits: only 8 exists."""
        from .baked_quant import quantize_field
        return quantize_field(self, bits)


def __getattr__(name):
    """the optimiser's names live in baked_train.py (which imports this module) and are reachable from here as well"""
    if name in ("BakedFieldOptimizer", "check_optimizer_args", "check_target_shape", "bias_corrected_rate", "check_tv_args",
                "fit_coarse_to_fine", "BrickFieldOptimizer", "brick_optimizer", "BRICK_TRAIN_VARIANTS", "BrickGridTrainer", "grid_trainer",
                "resample_bricks", "fit_coarse_to_fine_bricks"):
        from . import baked_train
        return getattr(baked_train, name)
    if name in ("QuantizedBrickField", "quantized_record_bytes", "quantize_bricks", "dequantize_bricks", "read_quantized_brick_file"):
        from . import baked_quant          # (it imports this module)
        return getattr(baked_quant, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _unpack_words(words, cells):
    """device int32 words of an occupancy bitfield -> bool [cx, cy, cz] on the device"""
    import torch
    shifts = torch.arange(32, device=words.device, dtype=torch.int32)
    bits = (words[:, None] >> shifts[None, :]) & 1
    n = cells[0] * cells[1] * cells[2]
    return bits.reshape(-1)[:n].reshape(cells).bool()


def bake(nerf, resolution=256, bounds=((-1.5,) * 3, (1.5,) * 3), net="fine", sh_degree=2, n_directions=None, sigma_threshold=0.0,
         slab_bytes=SLAB_BYTES, bricks=None, quantize=False):
    """NeRF.bake: see there.  The work list is processed in slabs: accumulator and compensation of ONE slab ([slab, K, 3] fp32 each,
    together at most slab_bytes) are summed over the directions and packed into the records before the next slab starts, so the
    working memory does not grow with the lattice.  Nothing waits for the GPU between slabs and directions; the one host read is the
    length of the work list.  slab_bytes is a tuning / diagnostic knob (tests force several slabs with it), not a promised part of the
    interface.  bricks = 4 or 8: the same work list in the same slabs is packed straight into a BrickBakedField (the dense record table
    is never allocated); the result is bake(...).compact(bricks) byte for byte.  quantize=True (needs bricks): the QuantizedBrickField
    bake(bricks=b).quantize(), byte for byte; the unquantised brick field exists transiently."""
    import torch
    from .runtime import _ptr, baked_project, occupancy_words_from_grid
    deg = check_degree(sh_degree)
    res, lo, hi = check_lattice_spec(resolution, bounds, deg)
    dirs, P = fit_directions(deg, n_directions)
    thr = check_threshold(sigma_threshold)
    brick = None if bricks is None else check_brick(bricks)
    if quantize and brick is None:
        raise ValueError("quantize=True needs bricks = 4 or 8: only a brick field can be quantised")
    if isinstance(slab_bytes, bool) or int(slab_bytes) != slab_bytes or int(slab_bytes) < 1:
        raise ValueError(f"slab_bytes must be a positive integer, got {slab_bytes!r}")
    n_net = nerf._field_net(net)
    ctx = nerf._ctx
    dev = torch.device(ctx.device)
    K, D = P.shape
    sigma = nerf.density_grid(res, (lo, hi), net)
    sigma = torch.where(sigma > thr, sigma, torch.zeros_like(sigma))
    field = BakedField._empty(sigma, res, lo, hi, deg, thr) if brick is None else BrickBakedField._empty(sigma, res, lo, hi, deg, thr, brick)
    # the work list: lattice points that are a corner of an occupied cell (a cell is occupied when a corner has sigma > 0)
    occ = field.occupied
    touched = torch.zeros(res, device=dev, dtype=torch.bool)
    cx, cy, cz = occ.shape
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                touched[a:a + cx, b:b + cy, c:c + cz] |= occ
    index = touched.reshape(-1).nonzero().reshape(-1)                  # int64, ascending
    n = int(index.numel())
    del touched, occ
    if n:
        lib = ctx.lib
        lo32 = torch.tensor(lo, device=dev, dtype=torch.float32)
        step32 = torch.tensor([(np.float32(h) - np.float32(l)) / np.float32(r - 1) for l, h, r in zip(lo, hi, res)], device=dev,
                              dtype=torch.float32)
        fit = torch.as_tensor(P.astype(np.float32)).to(dev).contiguous()
        dirs32 = torch.as_tensor(dirs.astype(np.float32)).to(dev).contiguous()
        slab = max(1, min(n, int(slab_bytes) // ((24 if D > 1 else 12) * K)))
        rgb = torch.empty((slab, 3), device=dev, dtype=torch.float32)
        acc = torch.empty((slab, K, 3), device=dev, dtype=torch.float32)
        comp = torch.empty_like(acc) if D > 1 else None            # the compensated sum over directions (knerf_baked_project)
        for s0 in range(0, n, slab):
            idx = index[s0:s0 + slab]
            m = int(idx.numel())
            ijk = torch.stack([idx // (res[1] * res[2]), (idx // res[2]) % res[1], idx % res[2]], dim=1).to(torch.float32)
            pts = torch.add(torch.mul(ijk, step32), lo32).contiguous()          # two roundings, as knerf_query_grid places its points
            a, e = acc[:m].zero_(), (None if comp is None else comp[:m].zero_())
            for j in range(D):
                dj = None if deg == 0 else dirs32[j]
                ctx._check(lib.knerf_query_points(ctx._ctx, ctx._stream(), n_net, _ptr(pts), _ptr(dj), 0, m, None, None, _ptr(rgb)))
                baked_project(rgb[:m], fit, j, a, e)
            field._pack(sigma, a, e, idx)
    if brick is not None:
        field._bake_sigma = None
    return field.quantize() if quantize else field
