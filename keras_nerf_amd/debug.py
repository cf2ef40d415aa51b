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
}
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
