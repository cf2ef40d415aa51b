"""NeRFTrainMonitor -- counterpart of reference keras_nerf/model/nerf/callback.py:8-226 (host-side observability).

Same artefacts: `<log_dir>/log.csv` (columns `epoch` + the 12 log keys, header written at epoch 0 only, one row per
`update_freq` epochs), `<log_dir>/model/` checkpoints (config json only at epoch 0), PNG panels `test_{i}_{epoch}.png`,
`test_sample_{i}_{epoch}.png`, `debug_{i}_{batch}.png` (verbose), and the resume rule `last_epoch = last CSV epoch + 1`
(the reference's reader skips the first data row when rebuilding its loss history, callback.py:38-46; kept).

Data parallel (one process per GPU): every rank keeps the loss history, only rank 0 renders panels and writes files (the
replicas hold identical weights and `fit` has already averaged the logs); the other ranks wait at a barrier so that nobody
runs ahead of a checkpoint that is still being written.  The barrier is reached even when rank 0's rendering, plotting or
writing raises (try/finally: the error then surfaces on rank 0 instead of as a collective time-out everywhere else), and the
"other test images" iterator walks a PRIVATE view of the dataset (own shuffle generator), so that its rank-0-only iteration
never advances the generator from which every rank derives the shared batch order.

OccupancyGridUpdater -- extension, no reference counterpart: empty-space skipping during fit, with occupancy grids kept in step with the
field as it learns (Instant-NGP's density EMA)."""
from __future__ import annotations

import logging
import os
from csv import DictReader, DictWriter

import numpy as np
import torch

from ... import parallel
from ...runtime import COARSE, FINE, check_grid_args, occupancy_box, occupancy_words_from_grid


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class NeRFTrainMonitor:
    def __init__(self, dataset, log_dir: str, batch_size: int, update_freq: int = 1, verbose: bool = False, plots: bool = True, **kwargs):
        self.dataset, self.log_dir, self.batch_size, self.update_freq, self.verbose = dataset, log_dir, batch_size, update_freq, verbose
        self.plots = plots
        self.model = None
        self.log_model_dir = os.path.join(log_dir, "model")
        os.makedirs(self.log_model_dir, exist_ok=True)
        self.coarse_log_list, self.val_coarse_log_list, self.fine_log_list, self.val_fine_log_list = [], [], [], []
        if self.verbose:
            self.coarse_log_list_batch, self.fine_log_list_batch = [], []
        self.last_epoch = 0
        self.log_csv = os.path.join(log_dir, "log.csv")
        if os.path.exists(self.log_csv):
            with open(self.log_csv, "r") as f:
                for i, row in enumerate(DictReader(f)):
                    if i > 0:
                        self.coarse_log_list.append(float(row["coarse_loss"])); self.val_coarse_log_list.append(float(row["val_coarse_loss"]))
                        self.fine_log_list.append(float(row["fine_loss"])); self.val_fine_log_list.append(float(row["val_fine_loss"]))
                        self.last_epoch = int(row["epoch"])
            self.last_epoch += 1
        for inputs in self.dataset.take(1):
            self.images, self.rays = inputs
            o, d, t = self.rays
            self.ray_origin, self.ray_direction, self.coarse_points = o[:batch_size], d[:batch_size], t[:batch_size]
        # rank-0-only iteration below must not touch the dataset's own generator (loader.py: the ranks' shared order)
        self._sample_view = self.dataset.private_view(seed=20240229) if hasattr(self.dataset, "private_view") else self.dataset
        self.dataset_iterator = iter(self._sample_view)
        self.dataset_iterator.get_next()

    def set_model(self, model):
        self.model = model

    # ---- plotting (matplotlib, Agg)
    def _panel(self, path, coarse, fine, gt, i, curves=None, title=None):
        if not self.plots:
            return
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        rows = 2 if curves else 1
        fig = plt.figure(figsize=(20, 5 * rows))
        gs = fig.add_gridspec(rows, 5)
        for k, (img, name, cmap) in enumerate([(coarse["image"], "Coarse Image", None), (coarse["depth"], "Coarse Depth", "inferno"),
                                               (fine["image"], "Fine Image", None), (fine["depth"], "Fine Depth", "inferno"),
                                               (gt, "Ground Truth", None)]):
            ax = fig.add_subplot(gs[0, k]); ax.imshow(np.clip(_np(img)[i][..., :3] if cmap is None else _np(img)[i], 0, None), cmap=cmap); ax.set_title(name)
        if curves:
            ax = fig.add_subplot(gs[1, :])
            for ys, color, style, label in curves:
                ax.plot(ys, color=color, linestyle=style, label=label)
            ax.legend(); ax.set_yscale("log"); ax.set_title(title)
        plt.savefig(path); plt.close(fig)

    def on_train_batch_end(self, batch, logs=None):
        if not self.verbose:
            return
        logging.debug(f"Batch {batch}: {logs}")
        self.coarse_log_list_batch.append(logs["coarse_loss"]); self.fine_log_list_batch.append(logs["fine_loss"])
        if not parallel.is_main():
            return
        coarse, fine = self.model.predict_and_render_images((self.ray_origin, self.ray_direction, self.coarse_points), outputs=("image", "depth"))
        curves = [(self.coarse_log_list_batch, "blue", "solid", "Coarse Train Loss"), (self.fine_log_list_batch, "orange", "solid", "Fine Train Loss")]
        for i in range(self.batch_size):
            self._panel(os.path.join(self.log_dir, f"debug_{i}_{batch}.png"), coarse, fine, self.images, i, curves, f"Loss Batch Plot: {batch}")

    def on_epoch_end(self, epoch, logs):
        self.coarse_log_list.append(logs["coarse_loss"]); self.val_coarse_log_list.append(logs["val_coarse_loss"])
        self.fine_log_list.append(logs["fine_loss"]); self.val_fine_log_list.append(logs["val_fine_loss"])
        if epoch % self.update_freq == 0 and not parallel.is_main():
            parallel.barrier()                                     # rank 0 is writing panels, log.csv and the checkpoint
        elif epoch % self.update_freq == 0:
            try:
                self._write_epoch(epoch, logs)
            finally:
                parallel.barrier()                                 # also when the writing failed: nobody is left waiting
        if self.verbose:
            self.coarse_log_list_batch, self.fine_log_list_batch = [], []

    def _write_epoch(self, epoch, logs):
        coarse, fine = self.model.predict_and_render_images((self.ray_origin, self.ray_direction, self.coarse_points), outputs=("image", "depth"))
        curves = [(self.coarse_log_list, "blue", "solid", "Coarse Train Loss"), (self.val_coarse_log_list, "blue", "dashed", "Coarse Val Loss"),
                  (self.fine_log_list, "orange", "solid", "Fine Train Loss"), (self.val_fine_log_list, "orange", "dashed", "Fine Val Loss")]
        for i in range(self.batch_size):
            self._panel(os.path.join(self.log_dir, f"test_{i}_{epoch}.png"), coarse, fine, self.images, i, curves, f"Loss Plot: {epoch}")
        try:                                                   # "Predict other test images" (callback.py:168-209)
            images, rays = self.dataset_iterator.get_next()
        except StopIteration:
            self.dataset_iterator = iter(self._sample_view)
            images, rays = self.dataset_iterator.get_next()
        o, d, t = [r[:self.batch_size] for r in rays]
        coarse, fine = self.model.predict_and_render_images((o, d, t), outputs=("image", "depth"))     # the panels show images and depths only
        for i in range(self.batch_size):
            self._panel(os.path.join(self.log_dir, f"test_sample_{i}_{epoch}.png"), coarse, fine, images, i)
        with open(self.log_csv, "a") as f:                     # callback.py:211-218
            new_logs = {"epoch": epoch}
            new_logs.update(logs)
            w = DictWriter(f, new_logs.keys())
            if epoch == 0:
                w.writeheader()
            w.writerow(new_logs)
        self.model.save_model(self.log_model_dir, weights_only=(epoch != 0))   # callback.py:220-222


class OccupancyGridUpdater:
    """Keeps one occupancy grid per net in step with the field during `fit` and trains behind them (NeRF.set_occupancy_training).

    After `warmup_steps` training steps, and every `update_every` steps after that, for each net: sigma on the (resolution + 1)^3
    lattice over `bounds` (NeRF.density_grid), state = max(decay * state, sigma) (the per-net density EMA, knerf_occupancy_decay_max),
    the grid of `state` (a cell occupied if a corner exceeds `threshold`, dilated by `dilation` cells; knerf_occupancy_from_grid) and
    attached to the net (KnerfContext.set_occupancy_words).  After the first update the option occupancy_train is on.  Everything is
    enqueued on the device: the host never waits for the GPU (no read-back, no blocking copy).  The grids stay attached after `fit`, so
    validation and later renders use them too (NeRF.clear_occupancy_grid detaches them).  Steps before the warm-up are the dense steps.

    With threshold 0 a cell dies only where the EMA of sigma is exactly 0 at all its lattice corners and in the dilation margin (DESIGN.md
    2.13).  Data parallel: every rank holds the same weights and builds the same grid with the same deterministic query."""

    def __init__(self, update_every=16, warmup_steps=256, resolution=128, bounds=((-1.5,) * 3, (1.5,) * 3), threshold=0.0, dilation=1,
                 decay=0.95, outside="occupied"):
        for name, v, lo in (("update_every", update_every, 1), ("warmup_steps", warmup_steps, 0)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
                raise ValueError(f"OccupancyGridUpdater: {name} must be an integer >= {lo}, got {v!r}")
        if isinstance(resolution, bool) or not isinstance(resolution, (int, np.integer)) or not 1 <= resolution <= 1024:
            raise ValueError(f"OccupancyGridUpdater: resolution must be an integer 1..1024 (cells per axis), got {resolution!r}")
        try:
            lo3, hi3 = bounds
        except (TypeError, ValueError):
            raise ValueError(f"OccupancyGridUpdater: bounds must be (lo[3], hi[3]); got {bounds!r}") from None
        _, self._lo, self._hi, _ = occupancy_box((int(resolution),) * 3, lo3, hi3, outside)
        check_grid_args(threshold, dilation, "OccupancyGridUpdater")
        if isinstance(decay, bool) or not isinstance(decay, (int, float, np.floating, np.integer)) or not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"OccupancyGridUpdater: decay must be a number in [0, 1], got {decay!r}")
        self.update_every, self.warmup_steps, self.resolution = int(update_every), int(warmup_steps), int(resolution)
        self.threshold, self.dilation, self.decay, self.outside = float(threshold), int(dilation), float(decay), outside
        self.model = None
        self.steps = 0              # training steps seen (over every fit this callback took part in)
        self.updates = 0            # grid updates made
        self._state = {}            # per net: the density EMA on the lattice (device)

    def set_model(self, model):
        self.model = model

    def due(self, steps: int) -> bool:
        """whether the grids are rebuilt once `steps` training steps have completed"""
        return steps >= self.warmup_steps and (steps - self.warmup_steps) % self.update_every == 0

    def on_train_begin(self, logs=None):
        if self.steps == 0 and self.due(0):         # warmup_steps = 0: a grid from the start
            self.update()

    def on_train_batch_end(self, batch, logs=None):
        self.steps += 1
        if self.due(self.steps):
            self.update()

    def update(self):
        """one update of both grids from the current weights (enqueued; nothing waits)"""
        m = self.model
        ctx = m._ctx
        res = self.resolution + 1
        for name, net in (("coarse", COARSE), ("fine", FINE)):
            sigma = m.density_grid(res, (self._lo, self._hi), name)
            state = self._state.get(name)
            if state is None:
                state = self._state[name] = torch.zeros_like(sigma)
            ctx.occupancy_decay_max(state, sigma, self.decay)
            words = occupancy_words_from_grid(state, self.threshold, self.dilation)
            ctx.set_occupancy_words(net, words, (self.resolution,) * 3, self._lo, self._hi, self.outside)
        if self.updates == 0:
            m.set_occupancy_training(True)
        self.updates += 1
