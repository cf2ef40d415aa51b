"""ctypes binding of libknerf_probe.so (include/knerf_debug.h): diagnostics for tests/ and tools/ ONLY.

The product path (runtime.py, model/, data/) never imports this module; tests/test_abi.py checks that, and that
libknerf_hip.so exports no `knerf_debug_*` symbol."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
PROBE_PATH = os.environ.get("KNERF_PROBE_LIB") or os.path.join(_HERE, "libknerf_probe.so")

_P = C.c_void_p
SIGNATURES = {
    "knerf_debug_table": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "knerf_debug_generic_plan": (C.c_int, [_P, _P, _P]),
    "knerf_debug_buffer": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "knerf_debug_probe": (C.c_int, [C.c_int, _P, _P, _P, _P]),
    "knerf_debug_write_probe": (C.c_int, [_P, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, _P]),
    "knerf_debug_read_probe": (C.c_int, [_P, C.c_int, C.c_longlong, C.c_int, _P, _P]),
    "knerf_debug_rate_probe": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, _P]),
    "knerf_debug_composite_train": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P, _P,
                                              _P, _P, _P, _P, _P, _P, C.c_int]),
    "knerf_debug_composite_objective": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P, _P,
                                                  _P, _P, _P, _P, _P, _P, C.c_int, C.POINTER(_lib.KnerfObjective), C.c_float, _P, _P]),
    "knerf_debug_compact_tiles": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "knerf_debug_generic_launch": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "knerf_debug_generic_wgrad_partial_floats": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "knerf_debug_generic_gemm": (C.c_int, [_P, _P]),
    "knerf_debug_generic_wgrad": (C.c_int, [_P, _P]),
    "knerf_debug_generic_check": (C.c_int, [C.c_int, _P]),
}


class DebugGemm(C.Structure):
    """knerf_debug_gemm of include/knerf_debug.h"""
    _fields_ = [("A", _P), ("a_elems", C.c_size_t), ("lda", C.c_int),
                ("Bt", _P), ("bt_elems", C.c_size_t), ("ldb", C.c_int),
                ("M", C.c_longlong), ("N", C.c_int), ("K", C.c_int),
                ("bias", _P), ("bias_elems", C.c_size_t), ("n_real", C.c_int),
                ("relu", C.c_int),
                ("mask_out", _P), ("mask_in", _P), ("mask_bytes", C.c_size_t), ("mask_cols", C.c_int),
                ("Cb", _P), ("cb_elems", C.c_size_t), ("ldc", C.c_int), ("c_col0", C.c_int),
                ("Cf", _P), ("cf_elems", C.c_size_t), ("ldcf", C.c_int),
                ("live", _P), ("n_live", C.c_longlong), ("live_dev", _P), ("live_dev_elems", C.c_size_t)]


class DebugWgrad(C.Structure):
    """knerf_debug_wgrad of include/knerf_debug.h"""
    _fields_ = [("X", _P), ("x_elems", C.c_size_t), ("ldx", C.c_int),
                ("Z", _P), ("z_elems", C.c_size_t), ("ldz", C.c_int),
                ("steps", C.c_longlong), ("N", C.c_int), ("K", C.c_int),
                ("grad", _P), ("grad_elems", C.c_size_t),
                ("w_off", C.c_int), ("b_off", C.c_int), ("n_real", C.c_int),
                ("n_seg", C.c_int), ("seg", C.c_int * 6),
                ("partial", _P), ("partial_elems", C.c_size_t),
                ("live", _P), ("n_live", C.c_longlong), ("live_dev", _P), ("live_dev_elems", C.c_size_t),
                ("selector", C.c_int)]
_probe = None


def load() -> C.CDLL:
    global _probe
    if _probe is None:
        _lib.load()                                    # the product library (and torch's HIP runtime) first
        if not os.path.exists(PROBE_PATH):
            raise _lib.KnerfError(f"{PROBE_PATH} is missing: run `python keras_nerf_amd/build.py`")
        lib = C.CDLL(PROBE_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _probe = lib
    return _probe


def debug_table(kind: int, shape: int = 0):
    """host-side packing / destination table `kind` of built-in trunk shape `shape` (see include/knerf_debug.h)"""
    import numpy as np
    lib = load()
    kind = int(kind) + 16 * int(shape)
    n = C.c_size_t(0)
    if lib.knerf_debug_table(kind, None, C.byref(n)) != 0:
        raise _lib.KnerfError("knerf_debug_table failed")
    out = np.empty(n.value, np.int32)
    if lib.knerf_debug_table(kind, out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)) != 0:
        raise _lib.KnerfError("knerf_debug_table failed")
    return out


def debug_buffer(ctx, which: int, net: int = 0):
    """uint8 torch view of a workspace of a runtime.KnerfContext (see knerf_debug_buffer)"""
    import torch
    from .runtime import _CudaView
    p, n = C.c_void_p(), C.c_size_t()
    if load().knerf_debug_buffer(ctx._ctx, int(net), int(which), C.byref(p), C.byref(n)) != 0:
        raise ValueError("debug_buffer: unknown or unallocated buffer (no pass has run yet, or it belongs to the other MLP path)")
    return torch.as_tensor(_CudaView(p.value, n.value, "|u1"), device=ctx.device)


def _dev_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def composite_train(raw, t, target, white, grad_scale, loss_scale, loss0=0.0, partial=False, flags=False, tiles=False,
                    count2_start=None, tile_off2=0):
    """The compositing kernel's training half on caller-made CUDA float32 tensors raw [R,S,4], t [R,S], target [R,3]
    (knerf_debug_composite_train).  Returns a dict of device tensors: image, depth, weights, draw, loss (started at loss0) and, as
    requested, loss_partial (partial=True: the deterministic loss form), tile_flags (flags=True), tile_list / tile_count
    (tiles=True) and tile_list2 / tile_count2 (count2_start = the second list's starting count; entries are index + tile_off2)."""
    import torch
    R, S = t.shape
    dev = raw.device
    assert raw.shape == (R, S, 4) and target.shape == (R, 3)
    assert all(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() for x in (raw, t, target))
    n_tiles = R * (S // 32)
    out = dict(image=torch.empty((R, 3), device=dev), depth=torch.empty((R,), device=dev), weights=torch.empty((R, S), device=dev),
               draw=torch.empty((R, S, 4), device=dev), loss=torch.full((1,), float(loss0), device=dev))
    if partial:
        out["loss_partial"] = torch.zeros(((R + 3) // 4,), device=dev)
    if flags:
        out["tile_flags"] = torch.full((max(n_tiles, 1),), -1, dtype=torch.int32, device=dev)
    if tiles:
        out["tile_list"] = torch.full((max(n_tiles, 1),), -1, dtype=torch.int32, device=dev)
        out["tile_count"] = torch.zeros((1,), dtype=torch.int32, device=dev)
    if count2_start is not None:
        assert tiles and count2_start >= 0
        out["tile_list2"] = torch.full((count2_start + max(n_tiles, 1),), -1, dtype=torch.int32, device=dev)
        out["tile_count2"] = torch.full((1,), int(count2_start), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = load().knerf_debug_composite_train(
        stream, _dev_ptr(raw), _dev_ptr(t), _dev_ptr(target), R, S, int(white), float(grad_scale), float(loss_scale),
        _dev_ptr(out["image"]), _dev_ptr(out["depth"]), _dev_ptr(out["weights"]), _dev_ptr(out["draw"]), _dev_ptr(out["loss"]),
        _dev_ptr(out.get("loss_partial")), _dev_ptr(out.get("tile_flags")), _dev_ptr(out.get("tile_list")),
        _dev_ptr(out.get("tile_count")), _dev_ptr(out.get("tile_list2")), _dev_ptr(out.get("tile_count2")), int(tile_off2))
    if rc != 0:
        raise _lib.KnerfError(f"knerf_debug_composite_train failed ({rc})")
    return out


def composite_objective(raw, t, target, white, grad_scale, loss_scale, objective, reg_scale, loss0=0.0, partial=False, flags=False,
                        tiles=False, count2_start=None, tile_off2=0):
    """composite_train on the EXTENDED compositing kernel (knerf_debug_composite_objective), always -- also for mse without a
    regulariser.  objective: a _lib.KnerfObjective (its `nets` is not read); reg_scale: inv_chunks / R.  Returns composite_train's dict
    plus terms [4] (photometric, squared error, distortion, entropy) and, with partial=True, terms_partial [4, ceil(R/4)]."""
    import torch
    R, S = t.shape
    dev = raw.device
    assert raw.shape == (R, S, 4) and target.shape == (R, 3)
    assert all(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() for x in (raw, t, target))
    n_tiles = R * (S // 32)
    out = dict(image=torch.empty((R, 3), device=dev), depth=torch.empty((R,), device=dev), weights=torch.empty((R, S), device=dev),
               draw=torch.empty((R, S, 4), device=dev), loss=torch.full((1,), float(loss0), device=dev), terms=torch.zeros((4,), device=dev))
    if partial:
        out["loss_partial"] = torch.zeros(((R + 3) // 4,), device=dev)
        out["terms_partial"] = torch.zeros((4, (R + 3) // 4), device=dev)
    if flags:
        out["tile_flags"] = torch.full((max(n_tiles, 1),), -1, dtype=torch.int32, device=dev)
    if tiles:
        out["tile_list"] = torch.full((max(n_tiles, 1),), -1, dtype=torch.int32, device=dev)
        out["tile_count"] = torch.zeros((1,), dtype=torch.int32, device=dev)
    if count2_start is not None:
        assert tiles and count2_start >= 0
        out["tile_list2"] = torch.full((count2_start + max(n_tiles, 1),), -1, dtype=torch.int32, device=dev)
        out["tile_count2"] = torch.full((1,), int(count2_start), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = load().knerf_debug_composite_objective(
        stream, _dev_ptr(raw), _dev_ptr(t), _dev_ptr(target), R, S, int(white), float(grad_scale), float(loss_scale),
        _dev_ptr(out["image"]), _dev_ptr(out["depth"]), _dev_ptr(out["weights"]), _dev_ptr(out["draw"]), _dev_ptr(out["loss"]),
        _dev_ptr(out.get("loss_partial")), _dev_ptr(out.get("tile_flags")), _dev_ptr(out.get("tile_list")),
        _dev_ptr(out.get("tile_count")), _dev_ptr(out.get("tile_list2")), _dev_ptr(out.get("tile_count2")), int(tile_off2),
        C.byref(objective), float(reg_scale), _dev_ptr(out["terms"]), _dev_ptr(out.get("terms_partial")))
    if rc != 0:
        raise _lib.KnerfError(f"knerf_debug_composite_objective failed ({rc})")
    return out


def compact_tiles(flags, period=1, real=1, stats=None):
    """knerf_debug_compact_tiles on a CUDA int32 tensor of flags: (list [n] int32 -- entries behind the count stay -1 --, count [1]
    int32); stats: an int64 [2] CUDA tensor whose two running totals the kernel adds to, or None"""
    import torch
    assert flags.is_cuda and flags.dtype == torch.int32 and flags.is_contiguous()
    n = flags.numel()
    lst = torch.full((n,), -1, dtype=torch.int32, device=flags.device)
    count = torch.full((1,), -1, dtype=torch.int32, device=flags.device)
    if stats is not None:
        assert stats.is_cuda and stats.dtype == torch.int64 and stats.numel() == 2
    stream = C.c_void_p(torch.cuda.current_stream(flags.device).cuda_stream)
    rc = load().knerf_debug_compact_tiles(_dev_ptr(flags), n, int(period), int(real), _dev_ptr(lst), _dev_ptr(count), _dev_ptr(stats), stream)
    if rc != 0:
        raise _lib.KnerfError(f"knerf_debug_compact_tiles failed ({rc})")
    return lst, count


def gemm_launch(M: int, N: int, K: int) -> dict:
    """which GEMM kernel and grid launch_gemm picks for (M, N, K) (knerf_debug_generic_launch; no device needed)"""
    out = (C.c_int32 * 8)()
    if load().knerf_debug_generic_launch(0, int(M), int(N), int(K), 0, out) != 0:
        raise ValueError(f"gemm_launch: bad shape {(M, N, K)}")
    ws, nt, gx, gy, lds, pitch = out[:6]
    tiles = M // 32
    return dict(kernel="ws" if ws else "stream", nt=nt, gx=gx, gy=gy, lds=lds, pitch=pitch,
                tiles_per_wave=-(-tiles // (8 * gx)) if ws else 1)


def wgrad_launch(K: int, N: int, steps: int, per_wave: bool = False) -> dict:
    """which weight-gradient kernel and grid launch_wgrad picks for a [K] x [N] layer over `steps` 32-row steps"""
    out = (C.c_int32 * 8)()
    if load().knerf_debug_generic_launch(1, int(steps), int(N), int(K), int(per_wave), out) != 0:
        raise ValueError(f"wgrad_launch: bad shape {(K, N, steps)}")
    coop, gx, gy, gz, kt, nt, n_slabs, slab = out[:8]
    return dict(kernel="coop" if coop else "wave", gx=gx, gy=gy, gz=gz, kt=kt, nt=nt, units=n_slabs, slab_floats=slab)


def wgrad_partial_floats(K: int, N: int, per_wave: bool = False) -> int:
    n = C.c_size_t(0)
    if load().knerf_debug_generic_wgrad_partial_floats(int(K), int(N), int(per_wave), C.byref(n)) != 0:
        raise ValueError(f"wgrad_partial_floats: bad shape {(K, N)}")
    return n.value


def _live_fields(args, live, tiles, device, ascending=False):
    """the live-tile list: a HOST int32 array (or None); checked here as well as in the library, which uploads it.  ascending: the
    deterministic weight gradient finds a unit's tiles by binary search"""
    import numpy as np
    import torch
    if live is None:
        args.live, args.n_live, args.live_dev, args.live_dev_elems = None, -1, None, 0
        return None
    host = np.ascontiguousarray(np.asarray(live, dtype=np.int32).reshape(-1))
    if host.size and (host.min() < 0 or host.max() >= tiles):
        raise ValueError("live list entries must lie in [0, tiles)")
    if ascending and host.size > 1 and (np.diff(host) <= 0).any():
        raise ValueError("the deterministic mode wants a strictly ascending live list")
    scratch = torch.full((host.size + 1,), -1, dtype=torch.int32, device=device)
    args.live = C.c_void_p(host.ctypes.data) if host.size else None
    args.n_live, args.live_dev, args.live_dev_elems = host.size, _dev_ptr(scratch), scratch.numel()
    return host, scratch                     # kept alive by the caller until the launch has been enqueued


def _bf16_ok(*ts):
    import torch
    return all(t is None or (t.is_cuda and t.dtype == torch.int16 and t.is_contiguous()) for t in ts)


def generic_gemm(A, lda, Bt, ldb, M, N, K, bias=None, n_real=0, relu=False, mask_out=None, mask_in=None, mask_cols=0,
                 Cb=None, ldc=0, c_col0=0, Cf=None, ldcf=0, live=None):
    """One launch_gemm on caller-made CUDA tensors (knerf_debug_generic_gemm): bf16 buffers are flat int16 tensors (bit patterns),
    bias / Cf float32, masks uint8.  live: None or a host array of 32-row tile indices.  Outputs are written in place.  Raises
    ValueError when the library refuses the arguments (nothing has been launched then)."""
    import torch
    assert _bf16_ok(A, Bt, Cb)
    assert all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in (bias, Cf))
    assert all(t is None or (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()) for t in (mask_out, mask_in))
    a = DebugGemm()
    a.A, a.a_elems, a.lda = _dev_ptr(A), A.numel(), int(lda)
    a.Bt, a.bt_elems, a.ldb = _dev_ptr(Bt), Bt.numel(), int(ldb)
    a.M, a.N, a.K = int(M), int(N), int(K)
    a.bias, a.bias_elems, a.n_real = _dev_ptr(bias), 0 if bias is None else bias.numel(), int(n_real)
    a.relu = int(bool(relu))
    mk = mask_out if mask_out is not None else mask_in
    a.mask_out, a.mask_in, a.mask_bytes, a.mask_cols = _dev_ptr(mask_out), _dev_ptr(mask_in), 0 if mk is None else mk.numel(), int(mask_cols)
    a.Cb, a.cb_elems, a.ldc, a.c_col0 = _dev_ptr(Cb), 0 if Cb is None else Cb.numel(), int(ldc), int(c_col0)
    a.Cf, a.cf_elems, a.ldcf = _dev_ptr(Cf), 0 if Cf is None else Cf.numel(), int(ldcf)
    keep = _live_fields(a, live, int(M) // 32, A.device)
    stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
    rc = load().knerf_debug_generic_gemm(stream, C.byref(a))
    del keep
    if rc == _lib.KNERF_ERR_INVALID:
        raise ValueError("knerf_debug_generic_gemm refused its arguments")
    if rc != 0:
        raise _lib.KnerfError(f"knerf_debug_generic_gemm failed ({rc})")


def generic_wgrad(X, ldx, Z, ldz, steps, K, N, grad, w_off, b_off, n_real, segs, partial=None, live=None, per_wave=False):
    """One launch_wgrad (+ the ordered reduce pass when `partial`, a float32 CUDA tensor of wgrad_partial_floats, is given) on
    caller-made CUDA tensors (knerf_debug_generic_wgrad).  segs: one or two (buffer col0, width, kernel row0).  grad is added to in
    place.  Raises ValueError when the library refuses the arguments."""
    import torch
    assert _bf16_ok(X, Z)
    assert all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in (grad, partial))
    a = DebugWgrad()
    a.X, a.x_elems, a.ldx = _dev_ptr(X), X.numel(), int(ldx)
    a.Z, a.z_elems, a.ldz = _dev_ptr(Z), Z.numel(), int(ldz)
    a.steps, a.N, a.K = int(steps), int(N), int(K)
    a.grad, a.grad_elems = _dev_ptr(grad), grad.numel()
    a.w_off, a.b_off, a.n_real = int(w_off), int(b_off), int(n_real)
    a.n_seg = len(segs)
    for i, sg in enumerate(segs[:2]):
        for j in range(3):
            a.seg[3 * i + j] = int(sg[j])
    a.partial, a.partial_elems = _dev_ptr(partial), 0 if partial is None else partial.numel()
    keep = _live_fields(a, live, int(steps), X.device, ascending=partial is not None)
    a.selector = int(bool(per_wave))
    stream = C.c_void_p(torch.cuda.current_stream(X.device).cuda_stream)
    rc = load().knerf_debug_generic_wgrad(stream, C.byref(a))
    del keep
    if rc == _lib.KNERF_ERR_INVALID:
        raise ValueError("knerf_debug_generic_wgrad refused its arguments")
    if rc != 0:
        raise _lib.KnerfError(f"knerf_debug_generic_wgrad failed ({rc})")
