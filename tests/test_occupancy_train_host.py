"""Training behind occupancy grids, host side, no GPU needed: the OccupancyGridUpdater's schedule (which steps rebuild the grids, none
before the warm-up) and argument checks, the NumPy mirror of the density EMA (knerf_occupancy_decay_max), argument errors of the
device-only grid route, NeRF.set_occupancy_training's validation, and the ABI entries."""
import numpy as np
import pytest

from keras_nerf_amd import runtime
from keras_nerf_amd.model.nerf.callback import OccupancyGridUpdater


def _steps(upd, n):
    done = []
    upd.update = lambda: done.append(upd.steps)
    upd.on_train_begin({})
    for b in range(n):
        upd.on_train_batch_end(b, {})
    return done


def test_updater_schedule():
    assert _steps(OccupancyGridUpdater(), 300) == [256, 272, 288]
    assert _steps(OccupancyGridUpdater(update_every=16, warmup_steps=256), 255) == []     # nothing before the warm-up
    assert _steps(OccupancyGridUpdater(update_every=5, warmup_steps=3), 14) == [3, 8, 13]
    assert _steps(OccupancyGridUpdater(update_every=4, warmup_steps=0), 9) == [0, 4, 8]  # warm-up 0: a grid before the first step
    u = OccupancyGridUpdater(update_every=10, warmup_steps=20)
    assert [s for s in range(60) if u.due(s)] == [20, 30, 40, 50]
    # a second fit continues the count
    u = OccupancyGridUpdater(update_every=4, warmup_steps=2)
    assert _steps(u, 3) == [2] and _steps(u, 4) == [6]


@pytest.mark.parametrize("kw", [dict(update_every=0), dict(update_every=1.5), dict(warmup_steps=-1), dict(warmup_steps=True),
                                dict(resolution=0), dict(resolution=1025), dict(resolution=64.0), dict(bounds=((0, 0, 0),)),
                                dict(bounds=((1, 1, 1), (0, 0, 0))), dict(threshold=float("nan")), dict(dilation=9),
                                dict(dilation=-1), dict(decay=1.5), dict(decay=-0.1), dict(decay="0.9"), dict(outside="inside")])
def test_updater_rejects_bad_arguments(kw):
    with pytest.raises(ValueError):
        OccupancyGridUpdater(**kw)


def test_decay_max_mirror():
    rng = np.random.default_rng(0)
    state = rng.random(1000).astype(np.float32) * 3
    sigma = np.maximum(rng.normal(size=1000), 0).astype(np.float32)
    out = runtime.occupancy_decay_max_reference(state, sigma, 0.95)
    assert out.dtype == np.float32
    assert np.array_equal(out, np.maximum(np.float32(0.95) * state, sigma))
    assert np.all(out >= sigma) and np.all(out >= np.float32(0.95) * state)
    # an EMA of a field that went empty decays geometrically; a field that stays dense keeps its maximum
    s = np.full(4, 8.0, np.float32)
    for _ in range(10):
        s = runtime.occupancy_decay_max_reference(s, np.zeros(4, np.float32), 0.5)
    assert np.array_equal(s, np.full(4, 8.0 / 1024, np.float32))
    assert np.array_equal(runtime.occupancy_decay_max_reference(s, np.full(4, 2.0, np.float32), 1.0), np.full(4, 2.0, np.float32))


def test_device_route_argument_errors():
    import torch
    cpu = torch.zeros((5, 5, 5), dtype=torch.float32)
    with pytest.raises(ValueError):
        runtime.occupancy_words_from_grid(cpu)                       # not a device tensor
    with pytest.raises(ValueError):
        runtime.occupancy_words_from_grid(torch.zeros((5, 5), dtype=torch.float32))
    with pytest.raises(ValueError):
        runtime.occupancy_decay_max(torch.zeros(4), torch.zeros(4), 0.9)      # host tensors
    for cells in ((0, 4, 4), (4, 4), (4, 4, 1025), (4.5, 4, 4), "abc"):
        with pytest.raises(ValueError):
            runtime.occupancy_box(cells, (-1,) * 3, (1,) * 3)
    with pytest.raises(ValueError):
        runtime.occupancy_box((4, 4, 4), (1,) * 3, (-1,) * 3)
    with pytest.raises(ValueError):
        runtime.occupancy_box((4, 4, 4), (-1,) * 3, (1,) * 3, "inside")
    assert runtime.occupancy_box((4, 5, 6), (-1,) * 3, (1,) * 3, "empty") == ((4, 5, 6), [-1.0] * 3, [1.0] * 3, 1)
    with pytest.raises(ValueError):
        runtime.check_grid_args(0.0, 9, "x")
    with pytest.raises(ValueError):
        runtime.check_grid_args(float("inf"), 1, "x")


def test_set_occupancy_training_validates_before_the_compile_check():
    from keras_nerf_amd.model.nerf.nerf import NeRF
    n = NeRF()
    for bad in (2, -1, 0.5, "yes", None):
        with pytest.raises(ValueError):
            n.set_occupancy_training(bad)
    for good in (True, False, 0, 1):
        with pytest.raises(RuntimeError):                              # not compiled
            n.set_occupancy_training(good)
    with pytest.raises(RuntimeError):
        n.occupancy_train_stats()


def test_the_abi_lists_the_new_entries():
    from keras_nerf_amd import _lib
    hdr = open(_lib.__file__.replace("keras_nerf_amd/_lib.py", "include/knerf.h")).read()
    for name in ("knerf_occupancy_train_stats", "knerf_occupancy_decay_max"):
        assert name in _lib.SIGNATURES and f"int {name}(" in hdr
    assert '"occupancy_train"' in hdr
