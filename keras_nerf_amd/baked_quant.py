"""The brick baked field with 8-bit SH coefficients (extension, no reference counterpart; PlenOctrees and SNeRG ship their SH
coefficients as 8-bit values with a scale): QuantizedBrickField, built by BrickBakedField.quantize, BakedField.quantize,
NeRF.bake(bricks=..., quantize=True) or QuantizedBrickField.load, rendered as it is; dequantize() leads back to a BrickBakedField.

The arithmetic is HIP (csrc/baked_quant.hip: knerf_baked_quantize_bricks, knerf_baked_dequantize_bricks, knerf_baked_render_qbricks;
include/knerf.h knerf_baked_qbricks holds the format).  The host-side mirrors of the codec (quantize_bricks, dequantize_bricks) and the
reader of format-3 files are NumPy and need no device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .baked import (BRICK_KEYS, BrickBakedField, _check, _ray_args, _stream, _unpack_words, brick_grid, check_brick, check_degree,
                    check_lattice_spec, check_render_args, check_table_size, check_threshold, n_coefficients, record_bytes)

QUANT_BITS = 8
EXPONENT_MIN, EXPONENT_MAX = -24, 9          # 2^-24: the fp16 subnormal spacing; 127 x 2^9 = 65024 <= 65504, the largest fp16 number
QLANES = {0: (1,), 1: (1,), 2: (1, 2), 3: (1, 4)}         # lanes per ray knerf_baked_render_qbricks is built for, per degree
QBRICK_KEYS = BRICK_KEYS + ("exponents", "quant_bits")


def quantized_record_bytes(sh_degree: int) -> int:
    """fp32 sigma + 3 K int8, padded to a power of two: 8 / 16 / 32 / 64"""
    return (8, 16, 32, 64)[check_degree(sh_degree)]


def coefficient_bands(sh_degree: int) -> np.ndarray:
    """the SH band l = floor(sqrt(k)) of each of the K coefficients"""
    return np.floor(np.sqrt(np.arange(n_coefficients(sh_degree)))).astype(np.int64)


def check_bits(bits) -> int:
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or int(bits) != QUANT_BITS:
        raise ValueError(f"only {QUANT_BITS}-bit quantisation exists, got bits = {bits!r}")
    return int(bits)


def quantize_bricks(brick_records, sh_degree):
    """NumPy mirror of knerf_baked_quantize_bricks: uint8 [n, b^3, record bytes] -> (quantised records uint8 [n, b^3, quantised record
    bytes], exponents uint32 [n]); the format is stated in include/knerf.h (knerf_baked_qbricks)"""
    deg = check_degree(sh_degree)
    K, rb, qb = n_coefficients(deg), record_bytes(deg), quantized_record_bytes(deg)
    rec = np.ascontiguousarray(brick_records, dtype=np.uint8)
    if rec.ndim != 3 or rec.shape[2] != rb:
        raise ValueError(f"brick records must be [n_bricks, b^3, {rb}] bytes for degree {deg}, got {rec.shape}")
    n, places = rec.shape[:2]
    co = np.ascontiguousarray(rec[:, :, 4:4 + 6 * K]).view(np.float16).reshape(n, places, K, 3).astype(np.float32)
    mag = np.where(np.isnan(co), np.float32(0), np.abs(co))
    band = coefficient_bands(deg)
    exps = np.zeros((n, 4), dtype=np.int64)
    scale = np.ones((n, 1, K, 1), dtype=np.float32)
    for l in range(deg + 1):
        M = mag[:, :, band == l, :].reshape(n, -1).max(axis=1) if n else np.zeros(0, np.float32)
        e = np.full(n, EXPONENT_MAX, dtype=np.int64)
        for cand in range(EXPONENT_MAX, EXPONENT_MIN - 1, -1):              # descending: the smallest e that still covers M is kept
            e = np.where(np.float32(127.0) * np.float32(2.0) ** np.float32(cand) >= M, cand, e)
        exps[:, l] = e
        scale[:, 0, band == l, 0] = (np.float32(2.0) ** (-e).astype(np.float32))[:, None]
    with np.errstate(invalid="ignore"):
        q = np.clip(np.rint(co * scale), -127.0, 127.0)
    q = np.where(np.isnan(co), np.float32(0), q).astype(np.int8)
    out = np.zeros((n, places, qb), dtype=np.uint8)
    out[:, :, :4] = rec[:, :, :4]
    out[:, :, 4:4 + 3 * K] = q.reshape(n, places, 3 * K).view(np.uint8)
    words = np.zeros(n, dtype=np.uint32)
    for l in range(deg + 1):
        words |= (exps[:, l] & 0xFF).astype(np.uint32) << np.uint32(8 * l)
    return out, words


def exponent_bytes(exponents, sh_degree) -> np.ndarray:
    """the used bytes of the exponent words: int64 [n, degree + 1]"""
    w = np.ascontiguousarray(exponents, dtype=np.uint32)
    return np.stack([((w >> np.uint32(8 * l)) & np.uint32(0xFF)).astype(np.uint8).view(np.int8).astype(np.int64)
                     for l in range(check_degree(sh_degree) + 1)], axis=-1)


def dequantize_bricks(qrecords, exponents, sh_degree):
    """NumPy mirror of knerf_baked_dequantize_bricks: (uint8 [n, b^3, quantised record bytes], uint32 [n]) -> ordinary brick records
    uint8 [n, b^3, record bytes]: sigma's bytes, the coefficients q 2^e as fp16 (exact), zero padding.  An exponent byte outside
    [-24, 9] is clamped into it, as the kernels do."""
    deg = check_degree(sh_degree)
    K, rb, qb = n_coefficients(deg), record_bytes(deg), quantized_record_bytes(deg)
    qr = np.ascontiguousarray(qrecords, dtype=np.uint8)
    if qr.ndim != 3 or qr.shape[2] != qb:
        raise ValueError(f"quantised records must be [n_bricks, b^3, {qb}] bytes for degree {deg}, got {qr.shape}")
    n, places = qr.shape[:2]
    ex = np.asarray(exponents)
    if ex.shape != (n,):
        raise ValueError(f"{n} bricks need {n} exponent words, got shape {ex.shape}")
    e = np.clip(exponent_bytes(ex, deg), EXPONENT_MIN, EXPONENT_MAX)[:, coefficient_bands(deg)]              # [n, K]
    q = np.ascontiguousarray(qr[:, :, 4:4 + 3 * K]).view(np.int8).reshape(n, places, K, 3).astype(np.float32)
    dec = (q * (np.float32(2.0) ** e.astype(np.float32))[:, None, :, None]).astype(np.float16)
    out = np.zeros((n, places, rb), dtype=np.uint8)
    out[:, :, :4] = qr[:, :, :4]
    out[:, :, 4:4 + 6 * K] = dec.reshape(n, places, 3 * K).view(np.uint8)
    return out


def read_quantized_brick_file(path) -> dict:
    """The arrays of a file QuantizedBrickField.save wrote (format 3), validated on the host: what baked.read_brick_file returns, with
    "records" in the quantised layout, and "exponents" uint32 [n_bricks].  ValueError on everything read_brick_file refuses of a
    format-2 file, on exponents of another dtype or length, on a used exponent byte outside [-24, 9] and on quant_bits != 8.  No
    device is touched."""
    with np.load(path) as z:
        missing = [k for k in QBRICK_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a quantised brick baked field of format 3 (missing {missing})")
        if np.ndim(z["format"]) != 0 or int(z["format"]) != 3:
            raise ValueError(f"{path}: baked-field format {z['format']!r} is not the quantised brick format 3")
        data = {k: z[k] for k in QBRICK_KEYS}
    for k in ("sh_degree", "brick", "sigma_threshold", "quant_bits"):
        if np.ndim(data[k]) != 0:
            raise ValueError(f"{path}: {k} must be a scalar, got shape {np.shape(data[k])}")
    for k in ("resolution", "lo", "hi"):
        if np.shape(data[k]) != (3,):
            raise ValueError(f"{path}: {k} must hold three values, got shape {np.shape(data[k])}")
    if any(data[k].dtype.kind not in "iu" for k in ("sh_degree", "brick", "resolution", "quant_bits")):
        raise ValueError(f"{path}: sh_degree, brick, resolution and quant_bits must be integers")
    if int(data["quant_bits"]) != QUANT_BITS:
        raise ValueError(f"{path}: quant_bits {int(data['quant_bits'])} is not {QUANT_BITS}")
    deg = check_degree(int(data["sh_degree"]))
    b = check_brick(int(data["brick"]))
    res, lo, hi = check_lattice_spec(tuple(int(r) for r in data["resolution"]), (data["lo"], data["hi"]), deg)
    thr = check_threshold(float(data["sigma_threshold"]))
    brick_of, records, words, exps = data["brick_of"], data["records"], data["words"], data["exponents"]
    B = brick_grid(res, b)
    if brick_of.dtype != np.int32 or brick_of.shape != B:
        raise ValueError(f"{path}: brick table {brick_of.dtype} {brick_of.shape} does not fit the {B} bricks of a {res} lattice")
    slots = brick_of.reshape(-1)[brick_of.reshape(-1) >= 0]
    if (brick_of < -1).any() or not np.array_equal(slots, np.arange(slots.size, dtype=np.int32)):
        raise ValueError(f"{path}: the brick table's slots are not 0..n-1 in ascending order (out of range, repeated or out of order)")
    n_bricks = max(int(slots.size), 1)
    cells = int(np.prod([r - 1 for r in res]))
    if records.dtype != np.uint8 or records.shape != (n_bricks, b ** 3, quantized_record_bytes(deg)) or words.dtype != np.int32 or \
            words.shape != ((cells + 31) // 32,):
        raise ValueError(f"{path}: records {records.dtype} {records.shape} / bits {words.dtype} {words.shape} do not fit {n_bricks} "
                         f"bricks of {b}^3 quantised records of degree {deg} on a {res} lattice")
    if exps.dtype != np.uint32 or exps.shape != (n_bricks,):
        raise ValueError(f"{path}: exponents {exps.dtype} {exps.shape} are not one uint32 word for each of {n_bricks} bricks")
    eb = exponent_bytes(exps, deg)
    if eb.size and (eb.min() < EXPONENT_MIN or eb.max() > EXPONENT_MAX):
        raise ValueError(f"{path}: an exponent byte lies outside [{EXPONENT_MIN}, {EXPONENT_MAX}] ({int(eb.min())}..{int(eb.max())})")
    check_table_size(n_bricks * b ** 3, deg)
    return {"records": records, "exponents": exps, "brick_of": brick_of, "words": words, "brick": b, "n_bricks": n_bricks,
            "resolution": res, "lo": lo, "hi": hi, "sh_degree": deg, "sigma_threshold": thr}


def _refuse(what):
    raise ValueError(f"{what} is not available on a QuantizedBrickField (refining a quantised field is out of scope): "
                     f"dequantize() gives the BrickBakedField that has it")


def quantize_field(field, bits=QUANT_BITS):
    """BrickBakedField.quantize: see there"""
    import torch
    from . import _lib
    from .runtime import _ptr
    check_bits(bits)
    if not isinstance(field, BrickBakedField):
        raise ValueError(f"quantize needs a BrickBakedField, got {type(field).__name__}")
    dev = field.device
    qrec = torch.empty((field.n_bricks, field.brick ** 3, quantized_record_bytes(field.sh_degree)), device=dev, dtype=torch.uint8)
    exps = torch.empty((field.n_bricks,), device=dev, dtype=torch.int32)
    _check(_lib.load().knerf_baked_quantize_bricks(_stream(dev), C.byref(field._c), _ptr(qrec), _ptr(exps)), "knerf_baked_quantize_bricks")
    return QuantizedBrickField(qrec, exps, field._brick_of, field._words, field.resolution, field.bounds, field.sh_degree, field.brick,
                               field.sigma_threshold)


class QuantizedBrickField:
    """A BrickBakedField whose SH coefficients are 8-bit values with one power-of-two scale per brick and SH band (include/knerf.h
    knerf_baked_qbricks): records of 8 / 16 / 32 / 64 bytes instead of 16 / 32 / 64 / 112.  Density, the brick table and the occupancy
    bits are the source field's, so empty-space skipping is as exact as ever.  render() marches the quantised bricks as they are; with
    lanes_per_ray=1 it gives the bits of dequantize().render(lanes_per_ray=1).  Optimising, resampling and pose refinement work on the
    BrickBakedField dequantize() returns."""

    def __init__(self, records, exponents, brick_of, words, resolution, bounds, sh_degree, brick=8, sigma_threshold=0.0):
        # uint8 [n_bricks, b^3, quantised record bytes], int32 [n_bricks] (the uint32 words' bits), int32 [Bx,By,Bz], int32 bits
        import torch
        self._records, self._exponents, self._brick_of, self._words = records, exponents, brick_of, words
        self.resolution = tuple(int(r) for r in resolution)
        self.bounds = (tuple(float(v) for v in bounds[0]), tuple(float(v) for v in bounds[1]))
        self.sh_degree = check_degree(sh_degree)
        self.brick = check_brick(brick)
        self.sigma_threshold = float(sigma_threshold)
        if records.dim() != 3 or tuple(records.shape[1:]) != (self.brick ** 3, quantized_record_bytes(self.sh_degree)) or \
                records.shape[0] < 1 or tuple(brick_of.shape) != brick_grid(self.resolution, self.brick) or \
                exponents.dtype != torch.int32 or tuple(exponents.shape) != (int(records.shape[0]),):
            raise ValueError(f"records {tuple(records.shape)} / exponents {exponents.dtype} {tuple(exponents.shape)} / brick table "
                             f"{tuple(brick_of.shape)} do not fit bricks of {self.brick}^3 quantised records of degree {self.sh_degree} "
                             f"on a {self.resolution} lattice")
        self.n_bricks = int(records.shape[0])
        from . import _lib
        bricks = _lib.KnerfBakedBricks(C.c_void_p(records.data_ptr()), C.c_void_p(brick_of.data_ptr()), C.c_void_p(words.data_ptr()),
                                       (C.c_int32 * 3)(*self.resolution), self.sh_degree, (C.c_float * 3)(*self.bounds[0]),
                                       (C.c_float * 3)(*self.bounds[1]), self.brick.bit_length() - 1, self.n_bricks)
        self._c = _lib.KnerfBakedQBricks(bricks, C.c_void_p(exponents.data_ptr()))

    @property
    def device(self):
        return self._records.device

    @property
    def brick_of(self):
        """int32 [Bx,By,Bz] on the device: the slot of every brick, -1 for an absent one"""
        return self._brick_of

    @property
    def exponents(self):
        """int32 [n_bricks] on the device holding the bits of the uint32 exponent words: byte l is band l's exponent (int8)"""
        return self._exponents

    @property
    def occupied(self):
        """bool [Rx-1,Ry-1,Rz-1] on the device: the cells with sigma > 0 at one of their corners"""
        return _unpack_words(self._words, tuple(r - 1 for r in self.resolution))

    @property
    def cell_size(self):
        return tuple((np.float32(h) - np.float32(l)) / (r - 1) for l, h, r in zip(self.bounds[0], self.bounds[1], self.resolution))

    @property
    def nbytes(self):
        """bytes on the device: records + exponents + brick table + occupancy bits"""
        return sum(int(t.numel()) * t.element_size() for t in (self._records, self._exponents, self._brick_of, self._words))

    def dequantize(self) -> BrickBakedField:
        """the BrickBakedField of the decoded coefficients (knerf_baked_dequantize_bricks; every decoded value is exactly an fp16
        number); it shares this field's brick table and bits.  dequantize().quantize() is this field byte for byte."""
        import torch
        from . import _lib
        from .runtime import _ptr
        records = torch.empty((self.n_bricks, self.brick ** 3, record_bytes(self.sh_degree)), device=self.device, dtype=torch.uint8)
        _check(_lib.load().knerf_baked_dequantize_bricks(_stream(self.device), C.byref(self._c), _ptr(records)),
               "knerf_baked_dequantize_bricks")
        return BrickBakedField(records, self._brick_of, self._words, self.resolution, self.bounds, self.sh_degree, self.brick,
                               self.sigma_threshold)

    def to_dense(self):
        """dequantize().to_dense(): the BakedField of the decoded records"""
        return self.dequantize().to_dense()

    # ---- persistence
    def save(self, path):
        """one .npz file at exactly `path` (no suffix is appended), format 3: the keys of BrickBakedField.save with the records in the
        quantised layout, and exponents (uint32 [n_bricks]) and quant_bits = 8"""
        with open(path, "wb") as f:
            np.savez(f, records=self._records.cpu().numpy(), exponents=self._exponents.cpu().numpy().view(np.uint32),
                     quant_bits=np.int32(QUANT_BITS), brick_of=self._brick_of.cpu().numpy(), words=self._words.cpu().numpy(),
                     brick=np.int32(self.brick), resolution=np.asarray(self.resolution, dtype=np.int32),
                     lo=np.asarray(self.bounds[0], dtype=np.float64), hi=np.asarray(self.bounds[1], dtype=np.float64),
                     sh_degree=np.int32(self.sh_degree), sigma_threshold=np.float64(self.sigma_threshold), format=np.int32(3))

    @classmethod
    def load(cls, path, device=None):
        """the field save(path) wrote; ValueError on a file that is not one (read_quantized_brick_file checks it before anything is
        uploaded)"""
        import torch
        d = read_quantized_brick_file(path)
        dev = torch.device(device if device is not None else "cuda")
        return cls(torch.as_tensor(d["records"]).to(dev), torch.as_tensor(d["exponents"].view(np.int32)).to(dev),
                   torch.as_tensor(d["brick_of"]).to(dev), torch.as_tensor(d["words"]).to(dev), d["resolution"], (d["lo"], d["hi"]),
                   d["sh_degree"], d["brick"], d["sigma_threshold"])

    # ---- rendering
    def render(self, origins, directions, near, far, step=None, white_background=False, termination=0.0,
               outputs=("image", "depth", "opacity"), skip_empty=True, stats=False, lanes_per_ray=0, background=None):
        """BrickBakedField.render on the quantised records (knerf_baked_render_qbricks): the same arguments, checks and result dict.
        lanes_per_ray: 0 = the library's choice, 1 = one ray per lane (any degree; the bits of dequantize().render(lanes_per_ray=1)),
        2 (degree 2) / 4 (degree 3) = a group of lanes per ray; the variants differ in summation order only."""
        if background is not None:      # a colour or [n,3]: the black-background launch composed on the host (render_over)
            from .baked import render_over
            return render_over(self, background, white_background, outputs, (origins, directions, near, far),
                               dict(step=step, termination=termination, skip_empty=skip_empty, stats=stats, lanes_per_ray=lanes_per_ray))
        import torch
        from . import _lib
        from .runtime import _ptr
        outs = check_render_args(step, termination, outputs)
        if lanes_per_ray != 0 and lanes_per_ray not in QLANES[self.sh_degree]:
            raise ValueError(f"lanes_per_ray must be 0 (default) or one of {QLANES[self.sh_degree]} for a quantised field of sh_degree "
                             f"{self.sh_degree}, got {lanes_per_ray!r}")
        dev = self.device
        o, d, n, h, (near_t, near0), (far_t, far0) = _ray_args(self, origins, directions, near, far, step)
        e = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
        res = {"image": e(n, 3) if "image" in outs else None, "depth": e(n) if "depth" in outs else None,
               "opacity": e(n) if "opacity" in outs else None}
        counter = torch.zeros(2, device=dev, dtype=torch.int64) if stats else None
        flags = (_lib.BAKED_WHITE_BACKGROUND if white_background else 0) | (_lib.BAKED_SKIP_EMPTY if skip_empty else 0) | \
            (int(lanes_per_ray) << _lib.BAKED_LANES_SHIFT)
        if n:
            _check(_lib.load().knerf_baked_render_qbricks(_stream(dev), C.byref(self._c), _ptr(o), _ptr(d), _ptr(near_t), _ptr(far_t), near0,
                                                          far0, n, h, float(termination), flags, _ptr(res["image"]), _ptr(res["depth"]),
                                                          _ptr(res["opacity"]), _ptr(counter)), "knerf_baked_render_qbricks")
        out = {k: v for k, v in res.items() if v is not None}
        if stats:
            out["stats"] = counter
        return out

    # ---- the field at points, on grids and as a mesh (baked_query.py): BakedField.query / density_grid / extract_mesh on the quantised records
    def query(self, points, directions=None, gradient=False, lanes_per_point=0):
        """BakedField.query on the quantised records (knerf_baked_query_qbricks); with lanes_per_point=1 the bits of
        dequantize().query(lanes_per_point=1)"""
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

    # ---- what a quantised field does not do
    def ray_gradients(self, *args, **kwargs):
        _refuse("ray_gradients")

    def optimizer(self, *args, **kwargs):
        _refuse("optimizer")

    def resample(self, *args, **kwargs):
        _refuse("resample")
