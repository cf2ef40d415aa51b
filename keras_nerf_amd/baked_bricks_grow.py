"""Growing a brick baked field as it is (extension, no reference counterpart): what baked_train.py has for a BakedField -- resampling onto
another lattice, the total-variation regulariser, coarse-to-fine fitting -- on the brick layout of BrickBakedField, and pruning while
training, so that a grid is refined stage by stage and goes sparse as it does without a tensor of the dense record table's size.

The arithmetic is HIP (csrc/baked_bricks_grow.hip: knerf_baked_resample_bricks_sigma and knerf_baked_resample_bricks are
knerf_baked_resample with a corner's record found through the brick table, knerf_baked_bricks_train_tv is knerf_baked_train_tv on the
rows of a brick optimiser; include/knerf.h holds the contract; both pairs share one text, csrc/baked_grow_common.h, and give the same
bits).  torch is used for device memory, streams and index plumbing only; that plumbing works brick slab by brick slab
(baked._brick_slabs) and on dense per-point SCALARS of at most 4 bytes (sigma, an int32 map from lattice point to row), never on dense
per-point rows.  Host reads: a brick count per brick table and n_slots per trainer.

The names live here and not on BrickBakedField, BrickFieldOptimizer or brick_optimizer, whose surfaces stay as they are.
"""
from __future__ import annotations

import ctypes as C

from .baked import (BakedField, BrickBakedField, _brick_points_device, _brick_slabs, _brick_table_device, _check, _stream, _unpack_words,
                    check_brick, check_lattice_spec, check_table_size, check_threshold, record_bytes)
from .baked_bricks_train import FLAG_SIGMA, FLAG_SLOT, BrickFieldOptimizer, brick_sigma, train_state
from .baked_train import TotalVariation, check_optimizer_args, check_stages, is_number, takes_depth_loss

CARRY_ROWS = 1 << 22          # rows whose columns move in one piece when a prune carries the optimiser's state


def _check_brick_field(field, what):
    """ValueError unless `field` is a BrickBakedField, with the way to one for the fields that are not"""
    from .baked_quant import QuantizedBrickField
    if isinstance(field, QuantizedBrickField):
        raise ValueError(f"{what} takes a BrickBakedField, got a QuantizedBrickField: dequantize() gives one")
    if isinstance(field, BakedField):
        raise ValueError(f"{what} takes a BrickBakedField, got a BakedField: compact() gives one (a BakedField has its own resample(), "
                         f"optimizer() and baked_train.fit_coarse_to_fine)")
    if not isinstance(field, BrickBakedField):
        raise ValueError(f"{what} takes a BrickBakedField, got {type(field).__name__}")


def stored_keys(brick_of):
    """int32 [n]: the linear index in the brick grid of every stored brick, ascending = in slot order (the inverse of brick_of)"""
    import torch
    return (brick_of.reshape(-1) >= 0).nonzero().reshape(-1).to(torch.int32)


def resample_bricks(field, resolution, sigma_threshold=None, brick=None):
    """`field` (a BrickBakedField) on another lattice (an int or three ints, 2..1025 points per axis) over the same box, as a
    BrickBakedField of `brick`^3 points per brick (default: the field's): field.to_dense().resample(resolution,
    sigma_threshold).compact(brick) byte for byte -- records, brick table, bits and brick count -- without either dense table.  Two
    launches: knerf_baked_resample_bricks_sigma writes the new sigma alone, dense fp32 (every new sigma <= sigma_threshold, default the
    field's own, stored as 0); the occupancy bits and the brick table are built from it, then knerf_baked_resample_bricks writes the
    records of the stored bricks.  A result without an occupied cell is the one all-zero brick.  `field` is left as it is."""
    import torch
    from . import _lib
    from .runtime import _ptr, occupancy_words_from_grid
    _check_brick_field(field, "resample_bricks")
    deg, dev = field.sh_degree, field.device
    res, _, _ = check_lattice_spec(resolution, field.bounds, deg)
    thr = field.sigma_threshold if sigma_threshold is None else check_threshold(sigma_threshold)
    b = field.brick if brick is None else check_brick(brick)
    sigma = torch.empty(res, device=dev, dtype=torch.float32)
    _check(_lib.load().knerf_baked_resample_bricks_sigma(_stream(dev), C.byref(field._c), (C.c_int32 * 3)(*res), thr, _ptr(sigma)),
           "knerf_baked_resample_bricks_sigma")
    words = occupancy_words_from_grid(sigma, 0.0, 0, what="resample_bricks")
    del sigma
    brick_of, n = _brick_table_device(_unpack_words(words, tuple(r - 1 for r in res)), res, b)
    check_table_size(max(n, 1) * b ** 3, deg)
    if n == 0:
        records = torch.zeros((1, b ** 3, record_bytes(deg)), device=dev, dtype=torch.uint8)
        return BrickBakedField(records, brick_of, words, res, field.bounds, deg, b, thr)
    records = torch.empty((n, b ** 3, record_bytes(deg)), device=dev, dtype=torch.uint8)
    out = BrickBakedField(records, brick_of, words, res, field.bounds, deg, b, thr)
    keys = stored_keys(brick_of)
    _check(_lib.load().knerf_baked_resample_bricks(_stream(dev), C.byref(field._c), C.byref(out._c), _ptr(keys), thr, _ptr(records)),
           "knerf_baked_resample_bricks")
    return out


def carried_rows(old_brick_of, old_flags, new_brick_of, new_flags, resolution, brick):
    """What a prune carries, as indices: for every row of the new train bricks (row = slot b^3 + place)
        old_row  int32 [n_new b^3]: the old row of the same lattice point where the point is a slot (flag bit 0) before AND after, else -1;
        sigma    bool  [n_new b^3]: old_row >= 0 and the point's sigma is trainable (flag bit 1) before and after.
    Index plumbing only, brick slab by brick slab over one dense int32 per lattice point; it runs on host tensors too."""
    import torch
    res, b = tuple(int(r) for r in resolution), int(brick)
    b3, dev = b ** 3, old_brick_of.device
    row_of = torch.full((res[0] * res[1] * res[2],), -1, device=dev, dtype=torch.int32)
    for s0, keys in _brick_slabs(old_brick_of, b, 4):
        lin, inside = _brick_points_device(keys, res, b)
        rows = torch.arange(s0 * b3, (s0 + int(keys.numel())) * b3, device=dev, dtype=torch.int32)
        ok = inside & ((old_flags[s0 * b3:(s0 + int(keys.numel())) * b3] & FLAG_SLOT) != 0)
        row_of[lin[ok]] = rows[ok]
    old_row = torch.full((int(new_flags.numel()),), -1, device=dev, dtype=torch.int32)
    sigma = torch.zeros((int(new_flags.numel()),), device=dev, dtype=torch.bool)
    for s0, keys in _brick_slabs(new_brick_of, b, 4):
        sl = slice(s0 * b3, (s0 + int(keys.numel())) * b3)
        lin, inside = _brick_points_device(keys, res, b)
        new = new_flags[sl]
        was = row_of[lin]
        ok = inside & ((new & FLAG_SLOT) != 0) & (was >= 0)
        was = torch.where(ok, was, torch.full_like(was, -1))
        old_row[sl] = was
        sigma[sl] = ok & ((new & FLAG_SIGMA) != 0) & ((old_flags[was.clamp(min=0).to(torch.int64)] & FLAG_SIGMA) != 0)
    return old_row, sigma


def carry_state(old_row, sigma, old, new):
    """new[r][1:] = old[old_row[r]][1:] where old_row[r] >= 0, and new[r][0] = old[old_row[r]][0] where sigma[r] (None: the sigma column
    is left as `new` has it); every other element of `new` stays.  old, new: fp32 rows [., 1 + 3 K].  In pieces of CARRY_ROWS rows."""
    import torch
    for r0 in range(0, int(old_row.numel()), CARRY_ROWS):
        was = old_row[r0:r0 + CARRY_ROWS]
        at = (was >= 0).nonzero().reshape(-1)
        src = was[at].to(torch.int64)
        new[r0:r0 + CARRY_ROWS][at, 1:] = old[src, 1:]
        if sigma is not None:
            at = sigma[r0:r0 + CARRY_ROWS].nonzero().reshape(-1)
            new[r0:r0 + CARRY_ROWS][at, 0] = old[was[at].to(torch.int64), 0]


class BrickGridTrainer(TotalVariation, BrickFieldOptimizer):
    """A BrickFieldOptimizer that can grow a grid (grid_trainer builds one): the total-variation regulariser of the dense optimiser
    (baked_train.TotalVariation: regularized, tv_weights(), regularize(), with the same meaning and, for the same values, the same
    gradient bits; train_step() runs it between accumulate() and apply() when a weight is > 0 and fit() then returns "tv_sigma" and
    "tv_sh" as well; with both weights 0 a step is BrickFieldOptimizer's, no further launch) and prune(), which re-supports the
    trainer on what the field has become and keeps Adam's state where it can."""

    @takes_depth_loss
    def __init__(self, source, learning_rate_sigma, learning_rate_sh, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dilation=0, step=None,
                 white_background=False, termination=0.0, lanes_per_ray=0, tv_sigma=0.0, tv_sh=0.0, tv_epsilon=1e-6, loss=None,
                 regularizers=None, background=None, opacity_loss=0.0, target_background=None, background_seed=0):
        self._set_tv(tv_sigma, tv_sh, tv_epsilon)
        super().__init__(source, learning_rate_sigma=learning_rate_sigma, learning_rate_sh=learning_rate_sh, beta_1=beta_1, beta_2=beta_2,
                         epsilon=epsilon, dilation=dilation, step=step, white_background=white_background, termination=termination,
                         lanes_per_ray=lanes_per_ray, loss=loss, regularizers=regularizers, background=background,
                         opacity_loss=opacity_loss, target_background=target_background, background_seed=background_seed)

    def _build(self, source) -> None:
        super()._build(source)
        self._keys = stored_keys(self.field._brick_of)

    def _tv_launch(self):
        from .runtime import _ptr
        return "knerf_baked_bricks_train_tv", (_ptr(self._keys), _ptr(self._flags), _ptr(self._master)), int(self._flags.numel())

    # ---- going sparse while training
    def counts(self):
        """{"n_bricks", "n_records", "n_slots"} of the trainer as it stands"""
        return {"n_bricks": self.field.n_bricks, "n_records": self.field.n_bricks * self.field.brick ** 3, "n_slots": self.n_slots}

    def prune(self, sigma_threshold=None, dilation=None):
        """Re-supports the trainer in place on what the field has become: the live field, the train bricks, the flags, the support and
        the records afterwards are exactly those of grid_trainer(self.finish(sigma_threshold), ..., dilation=dilation) (defaults: the
        field's threshold, this trainer's dilation, which a given one replaces from here on), so cells whose corners have all fallen
        to sigma <= sigma_threshold leave the support, and bricks without a support cell are dropped.  Adam's state is kept where it
        still means something: for a lattice point that is a slot before and after, the coefficient columns of master, m and v are the
        old row's bit for bit; the sigma column of m and v is carried where sigma is trainable before and after; master sigma is the
        new record's sigma (0 where it is not trainable); every other row starts as a fresh trainer's (moments zero).  iterations is kept, so the bias correction
        goes on.  A gradient that was accumulated and not yet applied is DISCARDED: prune between train steps.  While it runs the old
        and the new state exist side by side.  ValueError, with the trainer unchanged, when nothing would be left to optimise.
        Returns {"before": counts(), "after": counts()}."""
        import torch
        from .runtime import occupancy_words_from_grid
        dil = self.dilation if dilation is None else check_optimizer_args(self.learning_rate_sigma, self.learning_rate_sh, self.beta_1,
                                                                          self.beta_2, self.epsilon, dilation)[5]
        before = self.counts()
        source = self.finish(sigma_threshold)
        sigma = brick_sigma(source)[1]
        support = occupancy_words_from_grid(sigma, 0.0, dil, what="BrickGridTrainer.prune")
        del sigma
        brick_of, records, flags, master = train_state(source, support)          # (ValueError here: nothing has been changed yet)
        old_row, sigma_kept = carried_rows(self.field._brick_of, self._flags, brick_of, flags, source.resolution, source.brick)
        m, v = torch.zeros_like(master), torch.zeros_like(master)
        carry_state(old_row, None, self._master, master)
        carry_state(old_row, sigma_kept, self._m, m)
        carry_state(old_row, sigma_kept, self._v, v)
        self.dilation = dil
        self.field = BrickBakedField(records, brick_of, support, source.resolution, source.bounds, source.sh_degree, source.brick,
                                     source.sigma_threshold)
        self._flags, self._master, self._m, self._v = flags, master, m, v
        self._grad = torch.zeros_like(master)
        self._keys = stored_keys(brick_of)
        self.n_slots = int((flags & FLAG_SLOT).sum())
        self._c = self._state()
        return {"before": before, "after": self.counts()}


@takes_depth_loss
def grid_trainer(field, learning_rate_sigma, learning_rate_sh, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dilation=0, step=None,
                 white_background=False, termination=0.0, lanes_per_ray=0, tv_sigma=0.0, tv_sh=0.0, tv_epsilon=1e-6, loss=None,
                 regularizers=None, background=None, opacity_loss=0.0, target_background=None, background_seed=0):
    """A BrickGridTrainer over a COPY of a BrickBakedField's bricks: baked_train.brick_optimizer with the dense optimiser's
    total-variation keywords (tv_sigma, tv_sh: the weights of mean tv_sigma and mean tv_q, both >= 0; tv_epsilon > 0 under the root) and
    prune().  With both weights 0 it trains exactly as brick_optimizer's BrickFieldOptimizer does.  loss, regularizers: the objective, as
    BakedField.optimizer takes it; background, opacity_loss, target_background, background_seed: the rgba keywords, as there; depth_loss:
    the weight of the depth term, as there."""
    _check_brick_field(field, "grid_trainer")
    return BrickGridTrainer(field, learning_rate_sigma=learning_rate_sigma, learning_rate_sh=learning_rate_sh, beta_1=beta_1, beta_2=beta_2,
                            epsilon=epsilon, dilation=dilation, step=step, white_background=white_background, termination=termination,
                            lanes_per_ray=lanes_per_ray, tv_sigma=tv_sigma, tv_sh=tv_sh, tv_epsilon=tv_epsilon, loss=loss,
                            regularizers=regularizers, background=background, opacity_loss=opacity_loss,
                            target_background=target_background, background_seed=background_seed)


def check_prune_every(prune_every):
    """ValueError unless prune_every is None or a positive integer; returns it as None or int"""
    if prune_every is None:
        return None
    if not is_number(prune_every, integer=True) or int(prune_every) < 1:
        raise ValueError(f"prune_every must be a positive integer or None, got {prune_every!r}")
    return int(prune_every)


def fit_coarse_to_fine_bricks(field, batches, near, far, stages, sigma_threshold=None, prune_every=None, **trainer_kwargs):
    """baked_train.fit_coarse_to_fine on bricks: for every stage (resolution | None, steps) (baked_train.check_stages) the field is
    resampled onto `resolution` (resample_bricks with sigma_threshold; None keeps the lattice), a trainer is built on it
    (grid_trainer(field, **trainer_kwargs)), fit for `steps` batches -- with prune(sigma_threshold) after every `prune_every` steps that
    are not the stage's last, when prune_every is given -- and finished (finish(sigma_threshold)).  `batches` is consumed continuously,
    and its last_depth, where it has one, reaches every step (depth_loss= among the trainer's keywords).
    sigma_threshold None: every field's own threshold.

    Adam's moments are carried across a prune (BrickGridTrainer.prune) and NOT across a resample: a stage starts a fresh trainer.

    Returns (the finished BrickBakedField of the last stage, history): history["loss"] (and "tv_sigma", "tv_sh" when a weight is > 0) run
    over all stages; history["stages"] holds one {"resolution", "steps", "n_slots", "n_bricks", "n_records", "prunes"} per stage: the
    counts are the trainer's at the end of the stage, steps those actually run, prunes the list of what every prune() returned."""
    from .baked_train import StageBatches
    _check_brick_field(field, "fit_coarse_to_fine_bricks")
    todo = check_stages(stages)
    every = check_prune_every(prune_every)
    if sigma_threshold is not None:
        check_threshold(sigma_threshold)
    it = iter(batches)
    history = {"loss": [], "stages": []}
    for resolution, steps in todo:
        if resolution is not None:
            field = resample_bricks(field, resolution, sigma_threshold)
        opt = grid_trainer(field, **trainer_kwargs)
        done, prunes = 0, []
        while True:
            want = steps - done if every is None else min(every, steps - done)
            hist = opt.fit(StageBatches(batches, it, want), near, far)
            for key, values in hist.items():
                history.setdefault(key, []).extend(values)
            done += len(hist["loss"])
            if len(hist["loss"]) < want or done >= steps:                    # the batches ran out, or the stage is complete
                break
            prunes.append(opt.prune(sigma_threshold))
        history["stages"].append({"resolution": tuple(field.resolution), "steps": done, **opt.counts(), "prunes": prunes})
        field = opt.finish(sigma_threshold)
    return field, history
