"""Thin object wrapper over the C ABI (include/knerf.h): torch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C
import logging
import os
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import COARSE, FINE, KnerfConfig, KnerfError  # noqa: F401


class NonFiniteGradientError(ArithmeticError):
    """Counterpart of the InvalidArgumentError raised by tf.debugging.assert_all_finite (reference nerf.py:381-382)."""


_byref = C.byref      # (functions below use C for a channel count)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(x, device) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    return x.to(device=device, dtype=torch.float32).contiguous()


_GENERIC_SHAPES_WARNED = set()      # shapes already reported as "coverable by build.py --add-shape" (one warning each per process)

FUSED_WIDTHS = (64, 128, 256)       # csrc/layout.h: the trunk widths the fused kernels are written for


def padded_width(dense_units: int):
    """the width a dense_units is run at, or None (as it is).  Below 256: the next FUSED width -- 50 -> 64, 96 -> 128, 191 -> 256 (odd
    widths too: the reference's rgb_features layer has dense_units // 2 outputs, mlp.py:25, and so has the map).  Above 256 (general-shape
    kernels): the next multiple of 128 -- their GEMMs tile the output in blocks of 8, 4, 2 or 1 thirty-two-column tiles, whichever
    divides it, and every block re-reads the layer's input: 352 (11 tiles: eleven blocks) costs 24.9 ms per train chunk, 384 (three
    blocks of four) 13.1; 416 29.8 against 512's 18.0."""
    if dense_units < 2 or dense_units in FUSED_WIDTHS:
        return None
    if dense_units < FUSED_WIDTHS[-1]:
        return next(w for w in FUSED_WIDTHS if w >= dense_units)
    wide = -(-dense_units // 128) * 128
    return None if wide == dense_units else wide


def width_pad_index(n_layers: int, units: int, padded: int, skip_layer: int, xyz_dim: int, dir_dim: int) -> np.ndarray:
    """int64 [n_params(units)]: where parameter i of the REAL network (flat Keras order, mlp.py:11-27) sits in the flat parameters
    of the same network at width `padded`.  A kernel's h rows / h columns keep their index; the rows behind them ([h ; xyz_enc] of a
    concat layer, [features ; dir_enc] of rgb_features) move behind the padded h block."""
    from .model.nerf.mlp import layer_shapes
    real = layer_shapes(n_layers, units, skip_layer, xyz_dim, dir_dim)
    pad = layer_shapes(n_layers, padded, skip_layer, xyz_dim, dir_dim)
    idx, off = [], 0
    for (name, fi, fo), (_, fip, fop) in zip(real, pad):
        h_rows = {"layer_0": 0, "rgb": units // 2}.get(name, units)                 # leading rows that are h features of width `units`
        h_rows_p = {"layer_0": 0, "rgb": padded // 2}.get(name, padded)
        rows = np.arange(fi)
        rows_p = np.where(rows < h_rows, rows, rows - h_rows + h_rows_p)
        idx.append((off + rows_p[:, None] * fop + np.arange(fo)[None, :]).reshape(-1))
        off += fip * fop
        idx.append(off + np.arange(fo))
        off += fop
    return np.concatenate(idx).astype(np.int64)



class _CudaView:
    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


class KnerfContext:
    """Owns one knerf_ctx on the current CUDA(HIP) device."""

    def __init__(self, n_coarse=64, n_fine=128, pos_emb_xyz=10, pos_emb_dir=4, n_layers=8, dense_units=256, skip_layer=4,
                 white_background=False, oob="zero", lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7, device=None,
                 force_generic=None, options=None, encoded_widths=None, auto_build=None, pad_width=None):
        """force_generic: run the default MLP shape through the general-shape kernels as well (tests).  options: {name: value}
        for knerf_set_option.  encoded_widths = (xyz_dim, dir_dim): a stand-alone NeRFMLP of those two input widths
        (KNERF_FLAG_ENCODED_WIDTHS: weights and mlp_call only; pos_emb_* are ignored).  auto_build (default: $KNERF_AUTO_BUILD): a
        shape the fused kernels COULD cover but the loaded library does not hold is compiled for them on first use (hipcc, a few
        minutes once per shape; the build is kept in keras_nerf_amd/build_auto_*/) instead of running on the general-shape kernels.
        pad_width (default on; $KNERF_NO_WIDTH_PAD=1 turns it off): a dense_units below 256 that is not 64 / 128 / 256 runs on the
        FUSED kernels of the next of those widths with zero-padded weights -- an exact identity (padded neurons have zero kernel and
        bias: their activations, every gradient that touches them and hence their Adam updates are exactly zero; `_set_up_padding`) --
        whenever the library holds (or auto_build builds) that shape; set_weights / get_weights / grads() speak the REAL layout,
        weights_view / grads_view expose the padded buffers (what a data-parallel broadcast / all-reduce needs).  The LIBRARY reads no environment variables; for tools and sweeps this wrapper translates
        KNERF_FORCE_GENERIC, KNERF_WGRAD_GROUP_MAX, KNERF_WGRAD_GROUP_GB, KNERF_WGRAD_COSTS ("c0,...,c<n_layers>": one per weight-gradient job), KNERF_DETERMINISTIC and
        KNERF_SKIP_DEAD_TILES, KNERF_MERGE_CHUNK_RAYS, KNERF_MERGE_RENDER_RAYS into the config flag / options below (explicit arguments win)."""
        self._ctx = C.c_void_p()
        if not torch.cuda.is_available():
            raise KnerfError("keras_nerf_amd needs an MI355X (gfx950) GPU; there is no CPU path")
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        torch.cuda.set_device(self.device)
        if oob not in ("zero", "clamp"):
            raise ValueError("oob must be 'zero' or 'clamp'")
        if force_generic is None:
            force_generic = bool(os.environ.get("KNERF_FORCE_GENERIC"))
        flags = _lib.FLAG_FORCE_GENERIC if force_generic else 0
        if encoded_widths is not None:
            pos_emb_xyz, pos_emb_dir = (int(v) for v in encoded_widths)
            flags |= _lib.FLAG_ENCODED_WIDTHS
        self.cfg = KnerfConfig(n_coarse, n_fine, pos_emb_xyz, pos_emb_dir, n_layers, dense_units, skip_layer,
                               int(bool(white_background)), int(oob == "clamp"), lr, beta1, beta2, epsilon, flags)
        self.n_coarse, self.n_fine = n_coarse, n_fine
        self._pad_index = None          # torch int64 [real params] -> position in the padded flat parameters (width padding), or None
        if pad_width is None:
            pad_width = os.environ.get("KNERF_NO_WIDTH_PAD", "") in ("", "0")
        wide = padded_width(dense_units) if (pad_width and not force_generic and encoded_widths is None) else None
        # ... and where the library lacks this (n_layers, skip_layer) pair at that fused width but holds it one width up, that one: the
        # fused chain at 256 (3.4 ms per 8-layer chunk) still beats the general-shape kernels at 128 (3.8); two widths up it does not
        for cand in ([wide] + [w for w in FUSED_WIDTHS if wide < w <= 2 * wide][:1] if wide is not None else []):
            if self._set_up_padding(cand, auto_build if cand == wide else False):
                dense_units = cand                                      # from here on the context IS the padded shape
                break
        rc = 0 if self._ctx.value else self.lib.knerf_create(C.byref(self.cfg), C.byref(self._ctx))
        if rc != 0:
            msg = self.lib.knerf_last_error(None).decode()
            self._ctx = C.c_void_p()
            raise (ValueError if rc == _lib.KNERF_ERR_INVALID else KnerfError)(msg)
        if self._pad_index is None:
            self.param_count = int(self.lib.knerf_param_count_for(C.byref(self.cfg)))
        if not force_generic and encoded_widths is None and self.get_option("general_shape_path"):
            # a shape outside the library's list: where the fused kernels could cover it, build them (opt-in) or say how; else say what it costs
            eff = (padded_width(dense_units) if pad_width else None) or dense_units       # the width the fused kernels would run it at
            coverable = (eff in FUSED_WIDTHS and 3 <= n_layers <= 16 and skip_layer >= 1
                         and 1 <= pos_emb_xyz <= 16 and 1 <= pos_emb_dir <= 8 and not (eff == 256 and pos_emb_xyz == 16 and pos_emb_dir >= 5))
            spec = f"{n_layers},{skip_layer},{eff}" + ("" if (pos_emb_xyz, pos_emb_dir) == (10, 4) else f",{pos_emb_xyz},{pos_emb_dir}")
            if auto_build is None:
                auto_build = os.environ.get("KNERF_AUTO_BUILD", "") not in ("", "0")
            if coverable and auto_build and eff == dense_units:          # (a padded width was tried, and built if allowed, in _set_up_padding)
                self._rebuild_for(spec)
        if not force_generic and encoded_widths is None and self.get_option("general_shape_path"):
            # visible at the default log level when there is something the user can do about it, once per shape
            say = logging.info
            if coverable and spec not in _GENERIC_SHAPES_WARNED:
                _GENERIC_SHAPES_WARNED.add(spec)
                say = logging.warning
            say("NeRFMLP(n_layers=%d, dense_units=%d, skip_layer=%d), pos_emb %d/%d runs on the general-shape kernels (about 2x slower "
                "than the fused chain)%s", n_layers, dense_units, skip_layer, pos_emb_xyz, pos_emb_dir,
                f"; `python keras_nerf_amd/build.py --add-shape={spec}` builds the fused kernels for it (KNERF_AUTO_BUILD=1 does that on first use)" if coverable else "")
        opts = {}
        env = os.environ
        for key, name in (("KNERF_WGRAD_GROUP_MAX", "wgrad_group_max"), ("KNERF_WGRAD_GROUP_GB", "wgrad_group_gb"),
                          ("KNERF_DETERMINISTIC", "deterministic"), ("KNERF_SKIP_DEAD_TILES", "skip_dead_tiles"),
                          ("KNERF_MERGE_CHUNK_RAYS", "merge_chunk_rays"), ("KNERF_MERGE_RENDER_RAYS", "merge_render_rays")):
            if env.get(key) not in (None, ""):
                opts[name] = float(env[key])
        env_costs = {}
        if env.get("KNERF_WGRAD_COSTS"):          # one entry per weight-gradient job (n_layers + 1 of them); surplus entries are ignored
            for j, v in enumerate(env["KNERF_WGRAD_COSTS"].split(",")[:n_layers + 1]):
                env_costs[f"wgrad_cost{j}"] = float(v)
        opts.update(options or {})
        for k, v in opts.items():
            self.set_option(k, v)
        for k, v in env_costs.items():
            if k not in opts:
                try:
                    self.set_option(k, v)
                except ValueError:           # the context has fewer jobs than n_layers + 1 (general-shape path)
                    break

    def _set_up_padding(self, wide: int, auto_build) -> bool:
        """Try the network at width `wide` (zero-padded) on the fused kernels.  True: self._ctx is a fused context of the padded shape,
        self.cfg describes it, self.param_count / self._pad_index the real one.  False: nothing changed (the real shape then runs on
        the general-shape kernels as before).

        Why the padding is exact: a padded neuron j has a zero kernel column and zero bias, so z_j = 0 and h_j = relu(0) = 0 (a
        linear head layer: 0); the next layer's kernel rows for j are zero, so nothing reads it.  Backward: dz_j = [h_j > 0] (...) = 0
        at a relu, and W_next[j, :] . dz_next = 0 at a linear layer, so dW[:, j] = x^T dz_j = 0, db_j = 0 and dW_next[j, :] = h_j^T
        dz_next = 0: Adam's m and v stay 0 and its update 0 / (0 + eps) = 0 -- the zeros stay zeros, bit for bit, and the sums over the
        real neurons only ever gain exact zeros."""
        c = self.cfg
        cfg_p = KnerfConfig(c.n_coarse, c.n_fine, c.pos_emb_xyz, c.pos_emb_dir, c.n_layers, wide, c.skip_layer, c.white_background,
                            c.oob_clamp, c.lr, c.beta1, c.beta2, c.epsilon, c.flags)
        ctx = C.c_void_p()
        if self.lib.knerf_create(C.byref(cfg_p), C.byref(ctx)) != 0:
            return False
        real_cfg, real_ctx = self.cfg, self._ctx
        self.cfg, self._ctx = cfg_p, ctx
        generic = bool(self.get_option("general_shape_path")) and wide <= FUSED_WIDTHS[-1]      # (above 256 the general-shape kernels ARE the target)
        if generic:                                        # the padded shape is not in the library either: build it when allowed
            if auto_build is None:
                auto_build = os.environ.get("KNERF_AUTO_BUILD", "") not in ("", "0")
            coverable = (3 <= c.n_layers <= 16 and c.skip_layer >= 1 and 1 <= c.pos_emb_xyz <= 16
                         and 1 <= c.pos_emb_dir <= 8 and not (wide == 256 and c.pos_emb_xyz == 16 and c.pos_emb_dir >= 5))
            if coverable and auto_build:
                self._rebuild_for(f"{c.n_layers},{c.skip_layer},{wide}" + ("" if (c.pos_emb_xyz, c.pos_emb_dir) == (10, 4) else f",{c.pos_emb_xyz},{c.pos_emb_dir}"))
                generic = bool(self.get_option("general_shape_path"))
        if generic:
            self.lib.knerf_destroy(self._ctx)
            self.cfg, self._ctx = real_cfg, real_ctx
            return False
        self.param_count = int(self.lib.knerf_param_count_for(C.byref(real_cfg)))
        self.padded_param_count = int(self.lib.knerf_param_count_for(C.byref(cfg_p)))
        self.real_dense_units = int(real_cfg.dense_units)
        idx = width_pad_index(c.n_layers, int(real_cfg.dense_units), wide, c.skip_layer, 3 + 6 * c.pos_emb_xyz, 3 + 6 * c.pos_emb_dir)
        assert idx.size == self.param_count and int(idx.max()) < self.padded_param_count
        self._pad_index_host = idx
        self._pad_index = torch.as_tensor(idx, device=self.device)
        logging.info("dense_units=%d runs at width %d with zero-padded weights (exact) on the %s kernels", real_cfg.dense_units, wide,
                     "fused" if wide <= FUSED_WIDTHS[-1] else "general-shape")
        return True

    def _rebuild_for(self, spec: str):
        """KNERF_AUTO_BUILD: compile the fused kernels for this shape into their own library (build.py --variant=auto_<shape>
        --add-shape=<shape>; kept on disk, so the next process finds it built), load it beside the product library and re-create
        the context on it.  One process builds at a time (several ranks start together): a file lock around the build."""
        import fcntl
        from . import build as B
        variant = "auto_" + spec.replace(",", "_")
        lock_path = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), f".build_{variant}.lock")
        import torch.distributed as dist
        built = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), f"libknerf_hip_{variant}.so")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            # N ranks behind one file lock, two minutes of hipcc each turn, inside the process group's time-outs: not from a rank of a
            # running job.  A library built earlier (one process, before the job) is loaded as it is; otherwise the general-shape path.
            if not os.path.exists(built):
                logging.warning("KNERF_AUTO_BUILD: not compiling shape %s from rank %d of a %d-rank job (it runs on the general-shape kernels); "
                                "build it once beforehand: `python keras_nerf_amd/build.py --variant=%s --add-shape=%s`",
                                spec, dist.get_rank(), dist.get_world_size(), variant, spec)
                return
            path = built
            return self._adopt_library(path, spec)
        logging.warning("KNERF_AUTO_BUILD: building the fused kernels for shape %s (hipcc, a few minutes the first time)", spec)
        try:
            with open(lock_path, "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                try:
                    path = B.build(verbose=False, variant=variant, add_shapes=[spec])
                finally:
                    fcntl.flock(lock, fcntl.LOCK_UN)
        except Exception as e:                     # noqa: BLE001 -- no hipcc on this machine, a read-only tree, a shape that spills ...
            logging.warning("KNERF_AUTO_BUILD: building shape %s failed (%s: %s); it runs on the general-shape kernels", spec, type(e).__name__, e)
            return
        self._adopt_library(path, spec)

    def _adopt_library(self, path: str, spec: str):
        """re-create this context on the library at `path` (a build that holds shape `spec` for the fused kernels)"""
        self.lib.knerf_destroy(self._ctx)
        self._ctx = C.c_void_p()
        self.lib = _lib.load_path(path)
        rc = self.lib.knerf_create(C.byref(self.cfg), C.byref(self._ctx))
        if rc != 0:
            msg = self.lib.knerf_last_error(None).decode()
            self._ctx = C.c_void_p()
            raise KnerfError(f"KNERF_AUTO_BUILD: {path} refused the context: {msg}")
        if self.get_option("general_shape_path"):
            raise KnerfError(f"KNERF_AUTO_BUILD: {path} does not hold shape {spec}")

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self.lib.knerf_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- run-time options (include/knerf.h knerf_set_option)
    def set_option(self, name: str, value) -> None:
        self._check(self.lib.knerf_set_option(self._ctx, name.encode(), float(value)))

    def get_option(self, name: str) -> float:
        v = C.c_double()
        self._check(self.lib.knerf_get_option(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def tile_stats(self, reset: bool = True):
        """(live, total) 32-sample tiles seen by the dgrad launches since the last reset (skip_dead_tiles on)"""
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.knerf_tile_stats(self._ctx, self._stream(), C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value

    def tile_stats_net(self, reset: bool = True):
        """((live, total) of the coarse passes, (live, total) of the fine passes) since the last reset"""
        a, b = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        self._check(self.lib.knerf_tile_stats_net(self._ctx, self._stream(), a, b, int(reset)))
        return (a[0], b[0]), (a[1], b[1])

    def grad_diagnostics(self, wait: bool = True):
        """(non-zero entries of the last chunk's coarse gradient, of its fine gradient, steps published so far): the reference's
        tf.math.count_nonzero check (nerf.py:430-451); needs the option grad_diagnostics"""
        out = (C.c_int64 * 3)()
        self._check(self.lib.knerf_grad_diagnostics(self._ctx, self._stream(), int(wait), out))
        return int(out[0]), int(out[1]), int(out[2])

    # ---- helpers
    def _check(self, rc: int):
        if rc == 0:
            return
        msg = self.lib.knerf_last_error(self._ctx).decode()
        if rc == _lib.KNERF_ERR_NONFINITE:
            raise NonFiniteGradientError(msg)
        if rc == _lib.KNERF_ERR_INVALID:
            raise ValueError(msg)
        raise KnerfError(f"knerf error {rc}: {msg}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def f32(self, x) -> torch.Tensor:
        return _f32(x, self.device)

    # ---- weights
    def set_weights(self, net: int, flat):
        flat = np.ascontiguousarray(np.asarray(flat, dtype=np.float32).reshape(-1))
        if self._pad_index is not None:                # width padding: the real parameters into a zero vector of the padded layout
            if flat.size != self.param_count:
                raise ValueError(f"set_weights: {flat.size} values for a network of {self.param_count} parameters")
            wide = np.zeros(self.padded_param_count, np.float32)
            wide[self._pad_index_host] = flat
            flat = wide
        self._check(self.lib.knerf_set_weights(self._ctx, net, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size))

    def get_weights(self, net: int) -> np.ndarray:
        n = self.param_count if self._pad_index is None else self.padded_param_count
        out = np.empty(n, np.float32)
        self._check(self.lib.knerf_get_weights(self._ctx, net, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out if self._pad_index is None else out[self._pad_index_host]

    def grads(self, net: int) -> torch.Tensor:
        """the accumulated gradient of one net in the REAL flat layout (a copy): grads_view()'s half, un-padded where the width is padded"""
        g = self.grads_view()
        n = g.numel() // 2
        half = g[net * n:(net + 1) * n]
        return half.clone() if self._pad_index is None else half[self._pad_index]

    def weights_view(self, net: int) -> torch.Tensor:
        """torch view (no copy) of the library-owned fp32 master weights of one net"""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self.lib.knerf_weights_device(self._ctx, net, C.byref(p), C.byref(n)))
        return torch.as_tensor(_CudaView(p.value, n.value, "<f4"), device=self.device)

    def grads_view(self) -> torch.Tensor:
        """torch view (no copy) of the gradient accumulators [coarse | fine]: the buffer a DP step all-reduces"""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self.lib.knerf_grads_device(self._ctx, C.byref(p), C.byref(n)))
        return torch.as_tensor(_CudaView(p.value, n.value, "<f4"), device=self.device)

    def refresh_weights(self):
        self._check(self.lib.knerf_refresh_weights(self._ctx, self._stream()))

    # ---- forward
    def forward_chunk(self, net: int, o, d, t):
        o, d, t = self.f32(o), self.f32(d), self.f32(t)
        R, S = t.shape
        image = torch.empty((R, 3), device=self.device); depth = torch.empty((R,), device=self.device)
        weights = torch.empty((R, S), device=self.device)
        self._check(self.lib.knerf_forward_chunk(self._ctx, self._stream(), net, _ptr(o), _ptr(d), _ptr(t), R, S,
                                                 _ptr(image), _ptr(depth), _ptr(weights)))
        return image, depth, weights

    def sample_fine(self, t_coarse, w_coarse, u=None, seed=0, stream_id=0, ray_offset=0):
        t_coarse, w_coarse = self.f32(t_coarse), self.f32(w_coarse)
        u = None if u is None else self.f32(u)
        R = t_coarse.shape[0]
        out = torch.empty((R, self.n_coarse + self.n_fine), device=self.device)
        self._check(self.lib.knerf_sample_fine(self._ctx, self._stream(), _ptr(t_coarse), _ptr(w_coarse), _ptr(u), seed,
                                               stream_id, ray_offset, R, _ptr(out)))
        return out

    def render_chunk(self, o, d, t, u=None, seed=0, ray_offset=0, out=None):
        """out: optional dict of preallocated [R,...] tensors (c_image, c_depth, c_weights, f_image, f_depth, f_weights,
        t_fine); only the two images are mandatory"""
        o, d, t = self.f32(o), self.f32(d), self.f32(t)
        u = None if u is None else self.f32(u)
        R = t.shape[0]
        Na = self.n_coarse + self.n_fine
        if out is None:
            def e(*s):
                return torch.empty(s, device=self.device)
            out = dict(c_image=e(R, 3), c_depth=e(R), c_weights=e(R, self.n_coarse), f_image=e(R, 3), f_depth=e(R),
                       f_weights=e(R, Na), t_fine=e(R, Na))
        self._check(self.lib.knerf_render_chunk(self._ctx, self._stream(), _ptr(o), _ptr(d), _ptr(t), _ptr(u), seed,
                                                ray_offset, R, _ptr(out["c_image"]), _ptr(out.get("c_depth")),
                                                _ptr(out.get("c_weights")), _ptr(out["f_image"]), _ptr(out.get("f_depth")),
                                                _ptr(out.get("f_weights")), _ptr(out.get("t_fine"))))
        return out

    def render_batch(self, o, d, t, u=None, seed=0, ray_chunks=None, out=None):
        """the whole chunk loop of predict_and_render_images in one host call; `out` as in render_chunk but [N,...]
        (an optional out["t_fine"] [N, n_coarse+n_fine] receives the merged t-values)"""
        o, d, t = self.f32(o), self.f32(d), self.f32(t)
        u = None if u is None else self.f32(u)
        N = t.shape[0]
        Na = self.n_coarse + self.n_fine
        if out is None:
            def e(*s):
                return torch.empty(s, device=self.device)
            out = dict(c_image=e(N, 3), c_depth=e(N), c_weights=e(N, self.n_coarse), f_image=e(N, 3), f_depth=e(N), f_weights=e(N, Na))
        self._check(self.lib.knerf_render_batch(self._ctx, self._stream(), _ptr(o), _ptr(d), _ptr(t), _ptr(u), seed, N,
                                                int(ray_chunks or N), _ptr(out["c_image"]), _ptr(out.get("c_depth")),
                                                _ptr(out.get("c_weights")), _ptr(out["f_image"]), _ptr(out.get("f_depth")),
                                                _ptr(out.get("f_weights")), _ptr(out.get("t_fine"))))
        return out

    # ---- training
    def train_chunk(self, o, d, t, target, u=None, seed=0, ray_offset=0, inv_chunks=1.0, loss=None, c_image=None,
                    f_image=None):
        o, d, t, target = self.f32(o), self.f32(d), self.f32(t), self.f32(target)
        u = None if u is None else self.f32(u)
        self._check(self.lib.knerf_train_chunk(self._ctx, self._stream(), _ptr(o), _ptr(d), _ptr(t), _ptr(target), _ptr(u),
                                               seed, ray_offset, t.shape[0], float(inv_chunks), _ptr(loss), _ptr(c_image),
                                               _ptr(f_image)))

    def train_batch(self, o, d, t, target, u=None, seed=0, ray_chunks=None, loss=None, c_image=None, f_image=None):
        """the whole chunk loop of one train step (all arrays [N,...]; N % ray_chunks == 0)"""
        o, d, t, target = self.f32(o), self.f32(d), self.f32(t), self.f32(target)
        u = None if u is None else self.f32(u)
        n = t.shape[0]
        self._check(self.lib.knerf_train_batch(self._ctx, self._stream(), _ptr(o), _ptr(d), _ptr(t), _ptr(target), _ptr(u), seed, n,
                                               int(ray_chunks or n), _ptr(loss), _ptr(c_image), _ptr(f_image)))

    def apply_adam(self, check: bool = True):
        """finite check + 2x Keras-form Adam + accumulator reset, enqueued without waiting for the GPU.  check=True then
        waits and raises NonFiniteGradientError if the step was skipped (the reference's assert_all_finite, nerf.py:381-382);
        check=False leaves that to a later poll_nonfinite() at a point where the caller synchronises anyway."""
        self._check(self.lib.knerf_apply_adam(self._ctx, self._stream()))
        if check:
            self.poll_nonfinite(wait=True)

    def poll_nonfinite(self, wait: bool = False):
        self._check(self.lib.knerf_poll_nonfinite(self._ctx, self._stream(), int(wait)))

    def mlp_call(self, net: int, xyz_enc, dir_enc) -> torch.Tensor:
        """NeRFMLP.__call__ on already encoded inputs [n, xyz_dim] / [n, dir_dim]: raw [n,4] = (rgb, sigma)"""
        x, dd = self.f32(xyz_enc).contiguous(), self.f32(dir_enc).contiguous()
        n = x.shape[0]
        raw = torch.empty((n, 4), device=self.device, dtype=torch.float32)
        self._check(self.lib.knerf_mlp_call(self._ctx, self._stream(), int(net), _ptr(x), _ptr(dd), n, _ptr(raw)))
        return raw

    # ---- the trained field and its surface (extension: knerf_query_points / knerf_query_grid / knerf_marching_cubes)
    def query_points(self, net: int, xyz, dirs=None, raw=True, rgb=True):
        """the MLP at points xyz [n,3]; dirs None, [3] (shared) or [n,3].  raw=True: raw [n,4]; else (sigma [n], rgb [n,3] or None)"""
        x = self.f32(xyz).reshape(-1, 3)
        n = x.shape[0]
        dd, per_point = None, 0
        if dirs is not None:
            dd = self.f32(dirs)
            if dd.numel() == 3:
                dd = dd.reshape(3)
            else:
                dd, per_point = dd.reshape(-1, 3), 1
                if dd.shape[0] != n:
                    raise ValueError(f"query: {dd.shape[0]} directions for {n} points")
        e = lambda *s: torch.empty(s, device=self.device, dtype=torch.float32)
        if n == 0:
            return e(0, 4) if raw else (e(0), e(0, 3) if rgb else None)
        out_raw = e(n, 4) if raw else None
        sig = None if raw else e(n)
        col = e(n, 3) if (rgb and not raw) else None
        self._check(self.lib.knerf_query_points(self._ctx, self._stream(), int(net), _ptr(x), _ptr(dd), per_point, n, _ptr(out_raw),
                                                _ptr(sig), _ptr(col)))
        return out_raw if raw else (sig, col)

    def query_grid(self, net: int, resolution, lo, hi, direction=None, rgb=False):
        """sigma [R0,R1,R2] (and rgb [R0,R1,R2,3] when rgb) on the grid lo + idx * (hi - lo) / (R - 1) (include/knerf.h)"""
        res = (C.c_int32 * 3)(*[int(r) for r in resolution])
        lo3, hi3 = (C.c_float * 3)(*[float(v) for v in lo]), (C.c_float * 3)(*[float(v) for v in hi])
        dd = None if direction is None else self.f32(direction).reshape(3)
        shape = tuple(int(r) for r in resolution)
        sig = torch.empty(shape, device=self.device, dtype=torch.float32)
        col = torch.empty(shape + (3,), device=self.device, dtype=torch.float32) if rgb else None
        self._check(self.lib.knerf_query_grid(self._ctx, self._stream(), int(net), res, lo3, hi3, _ptr(dd), None, _ptr(sig), _ptr(col)))
        return sig, col


    # ---- empty-space skipping for rendering (extension: knerf_set_occupancy / knerf_occupancy_stats)
    def set_occupancy(self, net: int, occupied, lo=None, hi=None, outside: str = "occupied"):
        """Attach an occupancy grid to net `net`'s render passes: occupied = bool [cx, cy, cz] (NumPy or torch; 1..1024 cells per axis)
        over the box [lo, hi]; outside = "occupied" or "empty" (samples outside the box).  None detaches the net's grid.  Render passes
        of that net then run the MLP only on samples in occupied cells (include/knerf.h); training is not affected."""
        if net not in (COARSE, FINE):
            raise ValueError(f"net must be {COARSE} (coarse) or {FINE} (fine), got {net!r}")
        if occupied is None:
            self._check(self.lib.knerf_set_occupancy(self._ctx, self._stream(), int(net), None, None, None, None, 0))
            return
        words, cells, lo3, hi3, out_empty = occupancy_spec(occupied, lo, hi, outside)
        bits = torch.as_tensor(words.view(np.int32)).to(self.device)
        self._check(self.lib.knerf_set_occupancy(self._ctx, self._stream(), int(net), _ptr(bits), (C.c_int32 * 3)(*cells),
                                                 (C.c_float * 3)(*lo3), (C.c_float * 3)(*hi3), out_empty))

    def occupancy_stats(self, reset: bool = True):
        """((live, total) samples of the coarse render passes, (live, total) of the fine ones) since the last reset: live = samples in
        occupied cells (their MLP output is kept), total = samples of passes that had a grid"""
        a, b = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        self._check(self.lib.knerf_occupancy_stats(self._ctx, self._stream(), a, b, int(reset)))
        return (a[0], b[0]), (a[1], b[1])

    def set_occupancy_words(self, net: int, words: torch.Tensor, cells, lo, hi, outside: str = "occupied"):
        """Attach a grid that is already on the device: words = int32 / uint32 device tensor of ceil(cx cy cz / 32) packed words (as
        occupancy_words_from_grid returns them), cells = (cx, cy, cz).  The device-only route of set_occupancy: nothing is copied
        through the host and nothing waits for the GPU (the words are copied on the context's stream)."""
        if net not in (COARSE, FINE):
            raise ValueError(f"net must be {COARSE} (coarse) or {FINE} (fine), got {net!r}")
        cells3, lo3, hi3, out_empty = occupancy_box(cells, lo, hi, outside)
        need = (int(np.prod(cells3)) + 31) // 32
        if not isinstance(words, torch.Tensor) or words.dtype not in (torch.int32, torch.uint32) or words.dim() != 1 or \
                words.device != torch.device(self.device) or not words.is_contiguous():
            raise ValueError("set_occupancy_words: words must be a contiguous 1-D int32 tensor on the context's device")
        if words.numel() != need:
            raise ValueError(f"set_occupancy_words: {tuple(cells3)} cells need {need} words, got {words.numel()}")
        self._check(self.lib.knerf_set_occupancy(self._ctx, self._stream(), int(net), _ptr(words), (C.c_int32 * 3)(*cells3),
                                                 (C.c_float * 3)(*lo3), (C.c_float * 3)(*hi3), out_empty))

    def occupancy_train_stats(self, reset: bool = True):
        """((live, total) samples of the coarse TRAIN passes behind a grid, (live, total) of the fine ones) since the last reset
        (option occupancy_train; render passes are counted by occupancy_stats)"""
        a, b = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        self._check(self.lib.knerf_occupancy_train_stats(self._ctx, self._stream(), a, b, int(reset)))
        return (a[0], b[0]), (a[1], b[1])

    # ---- early ray termination for rendering (extension: options termination_threshold / termination_segment)
    def termination_stats(self, reset: bool = True):
        """((evaluated, total) samples of the coarse render passes with termination_threshold > 0, (evaluated, total) of the fine ones)
        since the last reset: evaluated = samples whose MLP output is kept (occupied and not terminated), total = every sample of those
        passes (include/knerf.h knerf_termination_stats)"""
        a, b = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        self._check(self.lib.knerf_termination_stats(self._ctx, self._stream(), a, b, int(reset)))
        return (a[0], b[0]), (a[1], b[1])

    def occupancy_decay_max(self, state: torch.Tensor, sigma: torch.Tensor, decay: float):
        """state = max(decay * state, sigma) in place on the context's stream (Instant-NGP's density EMA); both contiguous float32
        device tensors of the same size"""
        occupancy_decay_max(state, sigma, decay, stream=self._stream())

    def zero_grads(self):
        self._check(self.lib.knerf_zero_grads(self._ctx, self._stream()))

    @property
    def step(self) -> int:
        """optimizer steps applied so far (steps skipped for a non-finite gradient leave it once they have been polled)"""
        return int(self.lib.knerf_step_count(self._ctx))

    @step.setter
    def step(self, v: int):
        self._check(self.lib.knerf_set_step_count(self._ctx, int(v)))

    # ---- optimizer options and state (include/knerf.h knerf_set_optimizer / knerf_get_adam_state)
    def set_optimizer(self, opt=None, **kw):
        """knerf_set_optimizer: opt = a _lib.KnerfOptimizer, an optimizers.OptimizerSpec (anything with to_struct()), or the
        OptimizerSpec arguments as keywords (lr, schedule, clip, clip_arg, weight_decay).  Stream-ordered, callable between steps: the
        rate of the next step is re-derived on the device from the device-side step count.  beta1 / beta2 / epsilon stay the context's."""
        if opt is None:
            from .optimizers import OptimizerSpec
            opt = OptimizerSpec(**kw)
        elif kw:
            raise TypeError("set_optimizer: either an object or keywords")
        if not isinstance(opt, _lib.KnerfOptimizer):
            opt = opt.to_struct()
        self._check(self.lib.knerf_set_optimizer(self._ctx, self._stream(), C.byref(opt)))

    def get_optimizer(self) -> "_lib.KnerfOptimizer":
        """the record knerf_set_optimizer stored (canonical: what the chosen kinds do not read is zero)"""
        o = _lib.KnerfOptimizer()
        self._check(self.lib.knerf_get_optimizer(self._ctx, C.byref(o)))
        return o

    # ---- the objective (include/knerf.h knerf_set_objective)
    def set_objective(self, obj=None, **kw):
        """knerf_set_objective: obj = a _lib.KnerfObjective, or the arguments of losses.objective_from as keywords (loss, regularizers).
        Stream-ordered, callable between steps.  Mean squared error without a regulariser selects the plain compositing kernel."""
        if obj is None:
            from .losses import objective_from
            obj = objective_from(**kw)
        elif kw:
            raise TypeError("set_objective: either a record or keywords")
        self._check(self.lib.knerf_set_objective(self._ctx, self._stream(), C.byref(obj)))

    def get_objective(self) -> "_lib.KnerfObjective":
        """the record knerf_set_objective stored (canonical)"""
        o = _lib.KnerfObjective()
        self._check(self.lib.knerf_get_objective(self._ctx, C.byref(o)))
        return o

    def objective_terms(self) -> torch.Tensor:
        """device tensor [2, 4]: [coarse | fine] x [photometric, mean squared error, mean distortion, mean entropy] of the last
        train_batch (all zero under the plain objective); a stream-ordered copy, nothing waits"""
        out = torch.empty((2, 4), device=self.device, dtype=torch.float32)
        self._check(self.lib.knerf_objective_terms(self._ctx, self._stream(), _ptr(out)))
        return out

    def get_adam_state(self, net: int):
        """(m, v) of one net: Adam's slots in the REAL flat layout (as get_weights)"""
        n = self.param_count if self._pad_index is None else self.padded_param_count
        m, v = np.empty(n, np.float32), np.empty(n, np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.knerf_get_adam_state(self._ctx, self._stream(), int(net), m.ctypes.data_as(fp), v.ctypes.data_as(fp), n))
        return (m, v) if self._pad_index is None else (m[self._pad_index_host], v[self._pad_index_host])

    def set_adam_state(self, net: int, m, v):
        """the inverse of get_adam_state (width padding: the padded entries' slots are zero, as they always are)"""
        slots = []
        for name, x in (("m", m), ("v", v)):
            x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
            if x.size != self.param_count:
                raise ValueError(f"set_adam_state: {x.size} values of {name} for a network of {self.param_count} parameters")
            if self._pad_index is not None:
                wide = np.zeros(self.padded_param_count, np.float32)
                wide[self._pad_index_host] = x
                x = wide
            slots.append(x)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.knerf_set_adam_state(self._ctx, self._stream(), int(net), slots[0].ctypes.data_as(fp), slots[1].ctypes.data_as(fp),
                                                  slots[0].size))

    def generate_rays(self, c2w, focal, height, width, near, far, n_samples, noise=None, seed=0, stream_id=0):
        c2w = self.f32(c2w).reshape(-1, 4, 4)
        B = c2w.shape[0]
        noise = None if noise is None else self.f32(noise)
        o = torch.empty((B, height, width, 3), device=self.device); d = torch.empty_like(o)
        t = torch.empty((B, height, width, n_samples), device=self.device)
        self._check(self.lib.knerf_generate_rays(self._ctx, self._stream(), _ptr(c2w), _ptr(noise), seed, stream_id, B, height,
                                                 width, n_samples, float(focal), float(near), float(far), _ptr(o), _ptr(d),
                                                 _ptr(t)))
        return o, d, t

    def generate_rays_ext(self, c2w, focal, height, width, near, far, n_samples, ray_model, noise=None, seed=0, stream_id=0):
        """generate_rays under a ray model (_lib.KnerfRayModel, or None for pinhole rays with linear spacing): knerf_generate_rays_ext"""
        c2w = self.f32(c2w).reshape(-1, 4, 4)
        B = c2w.shape[0]
        noise = None if noise is None else self.f32(noise)
        o = torch.empty((B, height, width, 3), device=self.device); d = torch.empty_like(o)
        t = torch.empty((B, height, width, n_samples), device=self.device)
        self._check(self.lib.knerf_generate_rays_ext(self._ctx, self._stream(), _ptr(c2w), _ptr(noise), seed, stream_id, B, height,
                                                     width, n_samples, float(focal), float(near), float(far), _ptr(o), _ptr(d),
                                                     _ptr(t), None if ray_model is None else C.byref(ray_model)))
        return o, d, t

    def generate_rays_cam(self, c2w, camera, height, width, near, far, n_samples, ray_model=None, noise=None, seed=0, stream_id=0):
        """generate_rays_ext with a camera (data.cameras.CameraModel: one camera, or one per matrix of c2w) in place of the focal
        length: knerf_generate_rays_cam.  The camera's table is the caller's to have checked (CameraModel.check_invertible)."""
        c2w = self.f32(c2w).reshape(-1, 4, 4)
        B = c2w.shape[0]
        noise = None if noise is None else self.f32(noise)
        o = torch.empty((B, height, width, 3), device=self.device); d = torch.empty_like(o)
        t = torch.empty((B, height, width, n_samples), device=self.device)
        table, cs = camera.device_table(self.device), camera.c_struct()
        self._check(self.lib.knerf_generate_rays_cam(self._ctx, self._stream(), _ptr(c2w), _ptr(noise), seed, stream_id, B, height,
                                                     width, n_samples, _ptr(table), table.shape[0], C.byref(cs), float(near), float(far),
                                                     _ptr(o), _ptr(d), _ptr(t), None if ray_model is None else C.byref(ray_model)))
        return o, d, t

    def draw_ray_batch(self, images, c2w, focal, near, far, n_samples, seed, epoch, first, n_rays, noise=None, noise_stream=0,
                       want_index=False, ray_model=None, camera=None):
        """one batch of rays drawn over all pixels of `images` [V,H,W,3|4] (module-level draw_ray_batch, on this context)"""
        return draw_ray_batch(images, c2w, focal, near, far, n_samples, seed, epoch, first, n_rays, noise, noise_stream, want_index,
                              ctx=self, ray_model=ray_model, camera=camera)

    PROFILE_CLASSES = ("mlp_fwd_coarse", "mlp_fwd_fine", "composite", "sample_fine", "mlp_bwd_coarse", "mlp_bwd_fine",
                       "wgrad_coarse", "wgrad_fine", "adam_repack")

    def profile_enable(self, on: bool = True):
        self._check(self.lib.knerf_profile_enable(self._ctx, int(on)))

    def profile_read(self):
        """{class: (total_ms, launches)} since the last read"""
        n = len(self.PROFILE_CLASSES)
        ms = (C.c_double * n)(); cnt = (C.c_int64 * n)()
        self._check(self.lib.knerf_profile_read(self._ctx, ms, cnt, n))
        return {k: (ms[i], int(cnt[i])) for i, k in enumerate(self.PROFILE_CLASSES)}


def draw_ray_batch(images, c2w, focal, near, far, n_samples, seed, epoch, first, n_rays, noise=None, noise_stream=0,
                   want_index=False, ctx=None, ray_model=None, camera=None):
    """knerf_draw_ray_batch: slot i = pixel perm(seed, epoch)(first + i) of images [V,H,W,3|4] (float32, on the device) with camera
    matrices c2w [V,4,4].  Returns (o [n,3], d [n,3], t [n,n_samples], target [n,3]) and, with want_index, the flat pixel indices
    [n] (int64).  One launch on the current stream, nothing waits.  ctx: a KnerfContext, or None (the op needs none).
    ray_model: None -- the plain rays through knerf_draw_ray_batch -- or a _lib.KnerfRayModel (NDC rays, disparity spacing; a pinhole
    model with linear spacing gives the plain rays bit for bit) through knerf_draw_ray_batch_ext.
    camera: None, or a data.cameras.CameraModel (one camera, or one per view) that takes the place of `focal` (then unused, may be None):
    knerf_draw_ray_batch_cam, under the same ray_model.  Its table is the caller's to have checked (CameraModel.check_invertible)."""
    if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.float32 and images.dim() == 4):
        raise KnerfError("draw_ray_batch wants the images as one float32 [V,H,W,C] tensor on the device; there is no CPU path")
    dev = images.device
    images = images.contiguous()
    c2w = _f32(c2w, dev).reshape(-1, 4, 4)
    V, H, W, C = images.shape
    if c2w.shape[0] != V:
        raise ValueError(f"{V} images but {c2w.shape[0]} camera matrices")
    n = int(n_rays)
    if n <= 0:
        raise ValueError("n_rays must be positive")
    if noise is not None:
        noise = _f32(noise, dev)
        if tuple(noise.shape) != (n, n_samples):
            raise ValueError(f"noise must be [{n}, {n_samples}]")
    o = torch.empty((n, 3), device=dev); d = torch.empty_like(o); target = torch.empty_like(o)
    t = torch.empty((n, n_samples), device=dev)
    index = torch.empty((n,), device=dev, dtype=torch.int64) if want_index else None
    lib = ctx.lib if ctx is not None else _lib.load()
    head = (None if ctx is None else ctx._ctx, torch.cuda.current_stream(dev).cuda_stream, _ptr(images), _ptr(c2w), V, H, W, C)
    tail = (float(near), float(far), int(n_samples), int(seed), int(epoch),
            int(first), n, _ptr(noise), int(noise_stream), _ptr(o), _ptr(d), _ptr(t), _ptr(target), _ptr(index))
    if camera is not None:
        table, cs = camera.device_table(dev), camera.c_struct()
        rc = lib.knerf_draw_ray_batch_cam(*head, _ptr(table), table.shape[0], _byref(cs), *tail, None if ray_model is None else _byref(ray_model))
    else:
        args = (*head, float(focal), *tail)
        rc = lib.knerf_draw_ray_batch(*args) if ray_model is None else lib.knerf_draw_ray_batch_ext(*args, _byref(ray_model))
    if ctx is not None:
        ctx._check(rc)
    elif rc != 0:
        msg = f"knerf_draw_ray_batch failed ({rc}): {lib.knerf_last_error(None).decode(errors='replace')}"
        raise ValueError(msg) if rc == _lib.KNERF_ERR_INVALID else KnerfError(msg)
    return (o, d, t, target, index) if want_index else (o, d, t, target)


def marching_cubes(grid: torch.Tensor, threshold: float, lo, hi, normals: bool = True):
    """knerf_marching_cubes on a device fp32 grid [Rx,Ry,Rz] (contiguous): (vertices [V,3] f32, faces [F,3] int32, normals [V,3] or
    None), all on the grid's device.  Inside means sigma > threshold; an empty surface gives empty arrays."""
    lib = _lib.load()
    if not isinstance(grid, torch.Tensor) or grid.dtype != torch.float32 or grid.dim() != 3 or not grid.is_contiguous():
        raise ValueError("marching_cubes: the grid must be a contiguous float32 torch tensor [Rx, Ry, Rz]")
    if min(grid.shape) < 2:
        raise ValueError(f"marching_cubes: every resolution must be >= 2, got {tuple(grid.shape)}")
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3 or not all(np.float32(h) > np.float32(l) for l, h in zip(lo, hi)):
        raise ValueError(f"marching_cubes: need hi > lo on every axis, got {lo} / {hi}")
    dev = grid.device
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rx, ry, rz = (int(r) for r in grid.shape)
    lo3, hi3 = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
    nbytes, counts = C.c_size_t(0), (C.c_int64 * 2)()

    def chk(rc):
        if rc != 0:
            raise ValueError(f"knerf_marching_cubes failed ({rc}) on a [{rx},{ry},{rz}] grid") if rc == _lib.KNERF_ERR_INVALID else \
                KnerfError(f"knerf_marching_cubes failed ({rc})")
    chk(lib.knerf_marching_cubes(stream, None, rx, ry, rz, lo3, hi3, float(threshold), None, C.byref(nbytes), counts, None, None, None))
    ws = torch.empty((nbytes.value,), device=dev, dtype=torch.uint8)
    chk(lib.knerf_marching_cubes(stream, _ptr(grid), rx, ry, rz, lo3, hi3, float(threshold), _ptr(ws), C.byref(nbytes), counts, None, None,
                                 None))
    V, F = int(counts[0]), int(counts[1])
    verts = torch.empty((V, 3), device=dev, dtype=torch.float32)
    faces = torch.empty((F, 3), device=dev, dtype=torch.int32)
    nrm = torch.empty((V, 3), device=dev, dtype=torch.float32) if normals else None
    if V or F:
        chk(lib.knerf_marching_cubes(stream, _ptr(grid), rx, ry, rz, lo3, hi3, float(threshold), _ptr(ws), C.byref(nbytes), counts,
                                     _ptr(verts), _ptr(faces), _ptr(nrm)))
    return verts, faces, nrm


OCCUPANCY_OUTSIDE = ("occupied", "empty")


def pack_occupancy(occupied: np.ndarray) -> np.ndarray:
    """bool [cx, cy, cz] -> little-endian uint32 words: bit (i cy + j) cz + k is bit b % 32 of word b // 32 (padding bits 0)"""
    flat = np.ascontiguousarray(occupied, dtype=bool).reshape(-1)
    pad = -flat.size % 32
    if pad:
        flat = np.concatenate([flat, np.zeros(pad, dtype=bool)])
    return np.packbits(flat, bitorder="little").view("<u4").astype(np.uint32)


def unpack_occupancy(words, cells) -> np.ndarray:
    """the inverse of pack_occupancy: uint32 words -> bool [cx, cy, cz]"""
    w = np.ascontiguousarray(np.asarray(words).astype("<u4"))
    n = int(np.prod(cells))
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool).reshape(tuple(int(c) for c in cells))


def occupancy_box(cells, lo, hi, outside="occupied"):
    """validated (cells, lo[3], hi[3], outside_empty) of a grid's box; ValueError on bad arguments"""
    try:
        cells3 = tuple(cells)
    except TypeError:
        raise ValueError(f"occupancy: cells must be three integers, got {cells!r}") from None
    if len(cells3) != 3 or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= int(c) <= 1024 for c in cells3):
        raise ValueError(f"occupancy: cells must be three integers 1..1024, got {cells!r}")
    if outside not in OCCUPANCY_OUTSIDE:
        raise ValueError(f"occupancy: outside must be 'occupied' or 'empty', got {outside!r}")
    try:
        lo3, hi3 = [float(v) for v in lo], [float(v) for v in hi]
    except TypeError:
        raise ValueError(f"occupancy: lo and hi must be three numbers each, got {lo!r} / {hi!r}") from None
    if len(lo3) != 3 or len(hi3) != 3 or not all(np.isfinite(np.float32(v)) for v in lo3 + hi3) or \
            not all(np.float32(h) > np.float32(l) for l, h in zip(lo3, hi3)):
        raise ValueError(f"occupancy: need finite lo[3] < hi[3] on every axis, got {lo!r} / {hi!r}")
    return tuple(int(c) for c in cells3), lo3, hi3, int(outside == "empty")


def occupancy_spec(occupied, lo, hi, outside="occupied"):
    """validated (words uint32, cells, lo[3], hi[3], outside_empty) of a grid for knerf_set_occupancy; ValueError on bad arguments"""
    if isinstance(occupied, torch.Tensor):
        occupied = occupied.detach().cpu().numpy()
    occ = np.asarray(occupied)
    if occ.dtype != np.bool_:
        raise ValueError(f"occupancy: the grid must be boolean, got dtype {occ.dtype}")
    if occ.ndim != 3 or not all(1 <= c <= 1024 for c in occ.shape):
        raise ValueError(f"occupancy: the grid must be [cx, cy, cz] with 1..1024 cells per axis, got shape {occ.shape}")
    cells, lo3, hi3, out_empty = occupancy_box(occ.shape, lo, hi, outside)
    return pack_occupancy(occ), cells, lo3, hi3, out_empty


def occupancy_from_grid(sigma: torch.Tensor, threshold: float = 0.0, dilation: int = 1) -> np.ndarray:
    """knerf_occupancy_from_grid on a device fp32 lattice sigma [rx, ry, rz] (contiguous; 2..1025 per axis): bool [rx-1, ry-1, rz-1],
    a cell occupied if one of its 8 corners has sigma > threshold, then dilated by `dilation` cells (0..8, Chebyshev distance).  A
    heuristic: density between lattice points can be missed; the dilation is the margin."""
    words = occupancy_words_from_grid(sigma, threshold, dilation, what="occupancy_from_grid")
    return unpack_occupancy(words.cpu().numpy().view(np.uint32), tuple(int(r) - 1 for r in sigma.shape))


def check_lattice(sigma, threshold, dilation, what="occupancy_from_grid"):
    """ValueError unless sigma is a float32 device lattice [rx, ry, rz] (2..1025 per axis), dilation an integer 0..8 and threshold finite"""
    if not isinstance(sigma, torch.Tensor) or sigma.dtype != torch.float32 or sigma.dim() != 3 or not sigma.is_cuda:
        raise ValueError(f"{what}: sigma must be a float32 device tensor [rx, ry, rz]")
    if not all(2 <= r <= 1025 for r in sigma.shape):
        raise ValueError(f"{what}: need 2 <= resolution <= 1025 per axis (1..1024 cells), got {tuple(sigma.shape)}")
    check_grid_args(threshold, dilation, what)


def check_grid_args(threshold, dilation, what):
    if isinstance(dilation, bool) or int(dilation) != dilation or not 0 <= int(dilation) <= 8:
        raise ValueError(f"{what}: dilation must be an integer 0..8, got {dilation!r}")
    if not np.isfinite(float(threshold)):
        raise ValueError(f"{what}: threshold must be finite, got {threshold!r}")


def occupancy_words_from_grid(sigma: torch.Tensor, threshold: float = 0.0, dilation: int = 1, what="occupancy_words_from_grid") -> torch.Tensor:
    """occupancy_from_grid without the round trip through the host: the packed grid as a device int32 tensor of ceil(cells / 32)
    words (KnerfContext.set_occupancy_words takes it), enqueued on the current stream; nothing waits for the GPU"""
    check_lattice(sigma, threshold, dilation, what)
    sigma = sigma.contiguous()
    cells = tuple(int(r) - 1 for r in sigma.shape)
    words = torch.zeros(((int(np.prod(cells)) + 31) // 32,), device=sigma.device, dtype=torch.int32)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(sigma.device).cuda_stream)
    rc = lib.knerf_occupancy_from_grid(stream, _ptr(sigma), *(int(r) for r in sigma.shape), float(threshold), int(dilation), _ptr(words))
    if rc != 0:
        raise KnerfError(f"knerf_occupancy_from_grid failed ({rc})")
    return words


def occupancy_decay_max_reference(state: np.ndarray, sigma: np.ndarray, decay: float) -> np.ndarray:
    """NumPy mirror of knerf_occupancy_decay_max: max(fp32(decay * state), sigma)"""
    st = np.asarray(state, dtype=np.float32)
    return np.maximum(np.float32(decay) * st, np.asarray(sigma, dtype=np.float32)).astype(np.float32)


def _check_decay(state, sigma, decay):
    for name, x in (("state", state), ("sigma", sigma)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
            raise ValueError(f"occupancy_decay_max: {name} must be a contiguous float32 device tensor")
    if state.numel() != sigma.numel() or state.numel() == 0:
        raise ValueError(f"occupancy_decay_max: state and sigma must have the same non-zero size, got {state.numel()} / {sigma.numel()}")
    if state.device != sigma.device:
        raise ValueError("occupancy_decay_max: state and sigma must be on the same device")
    if isinstance(decay, bool) or not isinstance(decay, (int, float, np.floating, np.integer)) or not 0.0 <= float(decay) <= 1.0:
        raise ValueError(f"occupancy_decay_max: decay must be a number in [0, 1], got {decay!r}")


def occupancy_decay_max(state: torch.Tensor, sigma: torch.Tensor, decay: float, stream=None) -> torch.Tensor:
    """knerf_occupancy_decay_max: state = max(decay * state, sigma) in place, on `stream` (default: the current stream); returns state"""
    _check_decay(state, sigma, decay)
    lib = _lib.load()
    if stream is None:
        stream = C.c_void_p(torch.cuda.current_stream(state.device).cuda_stream)
    rc = lib.knerf_occupancy_decay_max(stream, _ptr(state), _ptr(sigma), int(state.numel()), float(decay))
    if rc != 0:
        raise KnerfError(f"knerf_occupancy_decay_max failed ({rc})")
    return state


# ---- the baked field (extension: knerf_baked_project / knerf_baked_pack / knerf_baked_render; keras_nerf_amd/baked.py holds the class)
def baked_project(rgb: torch.Tensor, fit: torch.Tensor, j: int, acc: torch.Tensor, comp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """knerf_baked_project: acc[n,K,3] += fit[k,j] rgb[n,c] in place on the current stream (one fma per element; with comp [n,K,3] the
    compensated sum of include/knerf.h); rgb [n,3], fit [K,D], all contiguous float32 device tensors; returns acc"""
    for name, x in (("rgb", rgb), ("fit", fit), ("acc", acc)) + ((("comp", comp),) if comp is not None else ()):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
            raise ValueError(f"baked_project: {name} must be a contiguous float32 device tensor")
    n = rgb.shape[0]
    if rgb.shape != (n, 3) or fit.dim() != 2 or acc.shape != (n, fit.shape[0], 3) or (comp is not None and comp.shape != acc.shape):
        raise ValueError(f"baked_project: need rgb [n,3], fit [K,D], acc [n,K,3]; got {tuple(rgb.shape)}, {tuple(fit.shape)}, {tuple(acc.shape)}")
    stream = C.c_void_p(torch.cuda.current_stream(acc.device).cuda_stream)
    rc = _lib.load().knerf_baked_project(stream, _ptr(rgb), _ptr(fit), int(fit.shape[0]), int(fit.shape[1]), int(j), n, _ptr(acc), _ptr(comp))
    if rc != 0:
        raise ValueError(f"knerf_baked_project refused its arguments (K = {fit.shape[0]}, D = {fit.shape[1]}, j = {j})") \
            if rc == _lib.KNERF_ERR_INVALID else KnerfError(f"knerf_baked_project failed ({rc})")
    return acc

