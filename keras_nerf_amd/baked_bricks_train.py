"""Optimising a brick baked field as it is (extension, no reference counterpart): BakedFieldOptimizer (baked_train.py) on the brick
layout of BrickBakedField, so that bake(bricks=) -> fine-tune -> finish() -> save never forms a tensor of the dense record table's size.

The arithmetic is HIP (csrc/baked_train.hip: knerf_baked_bricks_train_rays is knerf_baked_train_rays with a corner's address
formed through the brick table, knerf_baked_bricks_train_apply is knerf_baked_train_apply over the stored records; include/knerf.h holds
the contract).  torch is used for device memory, streams and the index plumbing of construction and finish() only; that plumbing works
brick slab by brick slab (baked._brick_slabs) and on dense per-point SCALARS of at most 4 bytes (sigma, bool masks), never on dense
per-point rows.  No step waits for the GPU.

What DESIGN.md 2.20 says about the dense optimiser holds here word for word (support, slots, trainable sigma); what differs (2.23):
  train bricks  the bricks that hold a corner of a support cell, numbered as a BrickBakedField numbers its bricks.  With dilation = 0
                they are the source's bricks; with dilation > 0 there can be more, and the added ones start as all-zero records;
  rows          master values, gradients and both Adam moments are fp32 [n_bricks b^3][1 + 3 K]: one row per STORED RECORD, the row's
                index is the record's index.  There is no slot table; a uint8 flag per record says whether it is a slot (bit 0) and
                whether its sigma is trainable (bit 1).  Rows of records that are no slot stay zero and are never touched.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .baked import (BrickBakedField, _brick_points_device, _brick_slabs, _brick_table_device, _stream, _unpack_words, check_table_size,
                    check_threshold, n_coefficients, record_bytes)
from .baked_train import GridOptimizer, is_number, slot_masks        # (the launches run in GridOptimizer, on baked_train._stream;
                                                                      # _stream above stays this module's name for the same lookup)

# lanes per ray knerf_baked_bricks_train_rays is built for, per degree: every variant of the dense gradient kernel builds without
# scratch with brick addressing as well (DESIGN.md 2.23 has hipcc's register counts)
BRICK_TRAIN_VARIANTS = {0: (1,), 1: (1, 2), 2: (1, 4), 3: (1, 4)}

FLAG_SLOT, FLAG_SIGMA = 1, 2            # bits of a record's flag: a corner of a support cell; sigma is trainable there


def check_brick_lanes(sh_degree, lanes_per_ray) -> int:
    """ValueError unless lanes_per_ray is 0 (the library's default) or one of BRICK_TRAIN_VARIANTS[sh_degree]"""
    if not is_number(lanes_per_ray, integer=True) or (int(lanes_per_ray) != 0 and int(lanes_per_ray) not in BRICK_TRAIN_VARIANTS[sh_degree]):
        raise ValueError(f"lanes_per_ray must be 0 (default) or one of {BRICK_TRAIN_VARIANTS[sh_degree]} for a brick optimiser of "
                         f"sh_degree {sh_degree}, got {lanes_per_ray!r}")
    return int(lanes_per_ray)


def brick_sigma(field, threshold=None):
    """sigma of a BrickBakedField two ways: (fp32 [n_bricks b^3] in record order, fp32 [Rx,Ry,Rz] dense with absent bricks reading as
    0).  threshold: every sigma <= threshold counts as 0 in both (None: as stored)."""
    import torch
    res, b = field.resolution, field.brick
    dense = torch.zeros((res[0] * res[1] * res[2],), device=field.device, dtype=torch.float32)
    stored = torch.zeros((field.n_bricks * b ** 3,), device=field.device, dtype=torch.float32)
    for s0, keys in _brick_slabs(field._brick_of, b, 4):
        m = int(keys.numel())
        lin, inside = _brick_points_device(keys, res, b)
        sg = field._records[s0:s0 + m, :, :4].contiguous().view(torch.float32).reshape(-1)
        if threshold is not None:
            sg = torch.where(sg > threshold, sg, torch.zeros_like(sg))
        stored[s0 * b ** 3:(s0 + m) * b ** 3] = sg
        dense[lin[inside]] = sg[inside]
    return stored, dense.reshape(res)


def train_state(source, support):
    """What a BrickFieldOptimizer starts from, given the support bits (int32 words over the cells): (brick_of int32 [Bx,By,Bz] of the
    train bricks, records uint8 [n, b^3, record bytes], flags uint8 [n b^3], master fp32 [n b^3, 1 + 3 K]).  The train bricks are
    those with a corner of a support cell; a brick the source stores is copied, any other starts as zero records.  Index plumbing
    only: it runs on host tensors too.  ValueError when the support is empty."""
    import torch
    res, b, deg, dev = source.resolution, source.brick, source.sh_degree, source.device
    K, rb, b3 = n_coefficients(deg), record_bytes(deg), b ** 3
    occ = _unpack_words(support, tuple(r - 1 for r in res))
    brick_of, n = _brick_table_device(occ, res, b)
    if n == 0:
        raise ValueError("the field has no occupied cell: there is nothing to optimise")
    check_table_size(n * b3, deg)
    touched, free = (mask.reshape(-1) for mask in slot_masks(occ, res))
    records = torch.zeros((n, b3, rb), device=dev, dtype=torch.uint8)
    flags = torch.zeros((n * b3,), device=dev, dtype=torch.uint8)
    master = torch.zeros((n * b3, 1 + 3 * K), device=dev, dtype=torch.float32)
    dst, src = records.view(torch.int32), source._records.view(torch.int32)                  # rows move as words, not as bytes
    source_of = source._brick_of.reshape(-1)
    for s0, keys in _brick_slabs(brick_of, b, rb + 4 * (1 + 3 * K)):
        m = int(keys.numel())
        old = source_of[keys].to(torch.int64)
        have = (old >= 0) & (old < source.n_bricks)
        dst[s0:s0 + m][have] = src[old[have]]
        lin, inside = _brick_points_device(keys, res, b)
        slot = touched[lin] & inside
        train = free[lin] & slot
        flags[s0 * b3:(s0 + m) * b3] = slot.to(torch.uint8) * FLAG_SLOT + train.to(torch.uint8) * FLAG_SIGMA
        rec = records[s0:s0 + m].reshape(-1, rb)
        sg = rec[:, :4].contiguous().view(torch.float32).reshape(-1)
        rows = master[s0 * b3:(s0 + m) * b3]
        rows[:, 0] = sg * train.to(torch.float32)                        # elsewhere sigma is 0 by the construction of the bits
        rows[:, 1:] = rec[:, 4:4 + 6 * K].contiguous().view(torch.float16).to(torch.float32)
    return brick_of, records, flags, master


def kept_bricks(live, sigma_stored, words, sigma_threshold):
    """finish() behind its one launch: the BrickBakedField of the bits `words` (a subset of live's support) with live's records and
    sigma_stored (fp32 [n_bricks b^3], already thresholded) in their sigma field.  The brick table is rebuilt from the bits, so a
    brick that no longer holds a touched point is dropped.  Index plumbing only: it runs on host tensors too."""
    import torch
    res, b, deg = live.resolution, live.brick, live.sh_degree
    rb, b3 = record_bytes(deg), b ** 3
    brick_of, n = _brick_table_device(_unpack_words(words, tuple(r - 1 for r in res)), res, b)
    records = torch.zeros((max(n, 1), b3, rb), device=live.device, dtype=torch.uint8)
    dst, src = records.view(torch.int32), live._records.view(torch.int32)
    sigma_words = sigma_stored.view(torch.int32).reshape(-1, b3)
    live_of = live._brick_of.reshape(-1)
    for s0, keys in _brick_slabs(brick_of, b, rb):
        # a cell with sigma > 0 at a corner is a support cell (that corner's sigma is trainable), so its 8 corners lie in live bricks
        old = live_of[keys].to(torch.int64)
        rows = src[old]
        rows[:, :, 0] = sigma_words[old]
        dst[s0:s0 + int(keys.numel())] = rows
    return BrickBakedField(records, brick_of, words, res, live.bounds, deg, b, sigma_threshold)


class BrickFieldOptimizer(GridOptimizer):
    """Adam on the records of a brick baked field (baked_train.brick_optimizer builds one): BakedFieldOptimizer's surface without the
    total-variation regulariser (the keywords, accumulate(), apply(), train_step() and fit() are baked_train.GridOptimizer's, over
    knerf_baked_bricks_train_rays[_ext|_rgba] and knerf_baked_bricks_train_apply).  `field` is the live BrickBakedField: it owns the
    records the optimiser rewrites, its bricks are the train bricks, its bits are the support, and it can be rendered at any time.
    The source field is left as it is."""

    _train_rays = "knerf_baked_bricks_train_rays"
    _check_lanes = staticmethod(check_brick_lanes)

    def _check_source(self, source) -> None:
        if not isinstance(source, BrickBakedField):
            raise ValueError(f"a brick optimiser is built on a BrickBakedField, got {type(source).__name__} (a BakedField has "
                             f"optimizer(), the dense BakedFieldOptimizer)")

    def _build(self, source) -> None:
        from .runtime import occupancy_words_from_grid
        sigma = brick_sigma(source)[1]
        support = occupancy_words_from_grid(sigma, 0.0, self.dilation, what="brick_optimizer")
        del sigma
        brick_of, records, self._flags, self._master = train_state(source, support)
        self.field = BrickBakedField(records, brick_of, support, source.resolution, source.bounds, source.sh_degree, source.brick,
                                     source.sigma_threshold)
        self.n_slots = int((self._flags & FLAG_SLOT).sum())                 # the one host read besides the brick count

    def _state(self):
        from . import _lib
        return _lib.KnerfBakedBricksTrain(self.field._c, C.c_void_p(self._grad.data_ptr()))

    def _apply_launch(self):
        from .runtime import _ptr
        return "knerf_baked_bricks_train_apply", (_ptr(self._flags),)

    # ---- views for tests and tools
    def _dense(self, per_record, dtype):
        """per_record [n_bricks b^3, ...] scattered onto the lattice [P, ...], zero where no brick is stored"""
        import torch
        f = self.field
        res, b3 = f.resolution, f.brick ** 3
        out = torch.zeros((res[0] * res[1] * res[2],) + tuple(per_record.shape[1:]), device=f.device, dtype=dtype)
        for s0, keys in _brick_slabs(f._brick_of, f.brick, 4 * max(1, int(np.prod(per_record.shape[1:])))):
            lin, inside = _brick_points_device(keys, res, f.brick)
            out[lin[inside]] = per_record[s0 * b3:(s0 + int(keys.numel())) * b3][inside].to(dtype)
        return out

    def gradients(self):
        """(g_sigma [Rx,Ry,Rz], g_coef [Rx,Ry,Rz,K,3]): dense fp32 copies of the accumulated gradient, zero outside the slots.  For
        tests on small lattices: these two are dense per-point rows, which nothing else here forms."""
        res, K = self.field.resolution, n_coefficients(self.field.sh_degree)
        g = self._dense(self._grad, self._grad.dtype)
        return g[:, 0].reshape(res), g[:, 1:].reshape(res + (K, 3))

    @property
    def slot_mask(self):
        """bool [Rx,Ry,Rz] on the device: the lattice points that have a slot"""
        import torch
        return self._dense((self._flags & FLAG_SLOT) != 0, torch.bool).reshape(self.field.resolution)

    @property
    def sigma_trainable(self):
        """bool [Rx,Ry,Rz] on the device: the lattice points whose sigma the optimiser may change"""
        import torch
        return self._dense((self._flags & FLAG_SIGMA) != 0, torch.bool).reshape(self.field.resolution)

    @property
    def nbytes(self):
        """bytes on the device: the live field (records + brick table + bits) and the state (flags, master, gradient, both moments)"""
        return self.field.nbytes + sum(int(t.numel()) * t.element_size() for t in (self._flags, self._master, self._grad, self._m, self._v))

    def finish(self, sigma_threshold=None):
        """An ordinary BrickBakedField from the live one: every sigma <= sigma_threshold (default: the field's own) stored as 0, the
        occupancy bits rebuilt from sigma (a subset of the support, so skipping stays exact), the brick table rebuilt from the bits
        and the kept bricks gathered.  It is BakedFieldOptimizer.finish().compact(brick) byte for byte.  The optimiser stays usable."""
        from .runtime import occupancy_words_from_grid
        f = self.field
        thr = f.sigma_threshold if sigma_threshold is None else check_threshold(sigma_threshold)
        stored, dense = brick_sigma(f, thr)
        words = occupancy_words_from_grid(dense, 0.0, 0, what="BrickFieldOptimizer.finish")
        del dense
        return kept_bricks(f, stored, words, thr)
