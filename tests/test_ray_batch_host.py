"""Host side of training on random ray batches (no GPU needed): the pixel permutation `keras_nerf_amd.data.ray_batch_permutation`
-- the NumPy statement the kernel of csrc/raybatch.hip is tested against (tests/test_gpu_ray_batch.py) -- and the bookkeeping of
`RayBatchDataset` with the device calls stubbed.

The statistical bounds are derived, not measured: 180.8 is the 1 - 1e-6 quantile of chi-square with 99 degrees of freedom
(scipy.stats.chi2.ppf(1 - 1e-6, 99)); for a uniformly random permutation two consecutive positions share a view with probability
(HW - 1) / (P - 1) ~ 1 / V and are neighbouring pixels with probability ~ 2 / P; two independent permutations agree in one position
on average."""
import types

import numpy as np
import pytest

from keras_nerf_amd.data import RayBatchDataset, ray_batch_permutation
from keras_nerf_amd.data.raybatch import rank_positions

SIZES = (1, 2, 3, 5, 1000, 2304, 1_638_400, 2 ** 20, 2 ** 20 + 1, 64_000_000)
BLOCK = 1 << 22


def _whole(P, seed, epoch):
    """(seen-exactly-once flags, longest walk) over every position of [0, P), in blocks"""
    seen, longest = np.zeros(P, bool), 0
    for a in range(0, P, BLOCK):
        out, walk = ray_batch_permutation(P, seed, epoch, np.arange(a, min(P, a + BLOCK)), return_walk=True)
        assert out.dtype == np.int64 and out.min() >= 0 and out.max() < P
        assert not seen[out].any() and len(np.unique(out)) == len(out), (P, seed, epoch)
        seen[out] = True
        longest = max(longest, int(walk.max()))
    return seen, longest


@pytest.mark.parametrize("P", SIZES)
def test_the_permutation_is_a_bijection_with_short_walks(P):
    for seed, epoch in ((0, 0), (0, 1), (7, 0), (7, 1)):
        seen, longest = _whole(P, seed, epoch)
        assert seen.all(), (P, seed, epoch)
        print(f"P={P} seed={seed} epoch={epoch}: longest cycle walk {longest}")
        assert longest <= 64, (P, seed, epoch, longest)


@pytest.mark.parametrize("P", [p for p in SIZES if p >= 1000 and p < 64_000_000])
def test_epochs_and_seeds_give_unrelated_permutations(P):
    pos = np.arange(P)
    a, b, c = (ray_batch_permutation(P, s, e, pos) for s, e in ((0, 0), (0, 1), (1, 0)))
    same_epoch, same_seed = int((a == b).sum()), int((a == c).sum())
    print(f"P={P}: {same_epoch} agreements between two epochs, {same_seed} between two seeds")
    assert same_epoch < 20 and same_seed < 20
    assert np.array_equal(a, ray_batch_permutation(P, 0, 0, pos))            # and a function of (P, seed, epoch, position) only
    assert np.array_equal(a[700:777], ray_batch_permutation(P, 0, 0, np.arange(700, 777)))


def test_batches_are_spread_over_the_views():
    V, HW, n = 100, 128 * 128, 4096
    P = V * HW
    worst = 0.0
    for seed in range(3):
        for epoch in range(3):
            pix = ray_batch_permutation(P, seed, epoch, np.arange(P))
            view = pix // HW
            for b in range(0, P // n, 50):
                counts = np.bincount(view[b * n:(b + 1) * n], minlength=V)
                chi2 = float(((counts - n / V) ** 2 / (n / V)).sum())
                worst = max(worst, chi2)
                assert chi2 < 180.8, (seed, epoch, b, chi2)
            same_view = float((view[1:] == view[:-1]).mean())
            d = pix[1:] - pix[:-1]
            neighbours = float(((np.abs(d) == 1) | (np.abs(d) == 128)).mean())
            print(f"seed {seed} epoch {epoch}: same view {same_view:.5f}, neighbouring pixels {neighbours:.2e}")
            assert abs(same_view - 1 / V) <= 0.001
            assert neighbours < 1e-4
    print(f"worst chi-square of the per-view counts over 72 batches: {worst:.1f}")


def test_rank_slices_tile_the_single_process_range():
    G = 32768
    for world in (1, 2, 4, 8):
        for step in (0, 3, 49):
            first0, n0 = rank_positions(step, G)
            got = []
            for r in range(world):
                first, n = rank_positions(step, G, r, world)
                assert n == G // world
                got.append(np.arange(first, first + n))
            cat = np.concatenate(got)
            assert len(np.unique(cat)) == G                                 # disjoint
            assert np.array_equal(cat, np.arange(first0, first0 + n0))       # and together the single-process range
    with pytest.raises(ValueError, match="not divisible"):
        rank_positions(0, 1000, 0, 3)


def test_arguments_are_checked():
    with pytest.raises(ValueError):
        ray_batch_permutation(0, 0, 0, [0])
    with pytest.raises(ValueError):
        ray_batch_permutation(2 ** 40, 0, 0, [0])
    with pytest.raises(ValueError):
        ray_batch_permutation(10, 0, 0, [10])
    assert ray_batch_permutation(1, 5, 9, [0]).tolist() == [0]


# ---- RayBatchDataset with the device stubbed
def _dataset(n_views=5, wh=24, rank=None, world=None, device_cache_gb=64.0):
    from keras_nerf_amd.data.loader import RayImageDataset
    loader = types.SimpleNamespace(image_width=wh, image_height=wh)
    rg = lambda rank=0: types.SimpleNamespace(focal_length=30.0, image_width=wh, image_height=wh, near=2.0, far=6.0, n_sample=8, seed=0)
    return RayImageDataset([f"img{i}" for i in range(n_views)], [np.eye(4)] * n_views, loader, rg, 1, rank=rank, world=world,
                           device_cache_gb=device_cache_gb)


@pytest.fixture
def drawn(monkeypatch):
    """the arguments of every draw_ray_batch call, with the resident cache and the kernel stubbed"""
    import keras_nerf_amd.runtime as rt
    calls = []

    def fake_draw(images, c2w, focal, near, far, n_samples, seed, epoch, first, n_rays, noise=None, noise_stream=0, want_index=False):
        calls.append(dict(seed=seed, epoch=epoch, first=first, n=n_rays, stream=noise_stream, n_samples=n_samples))
        return "o", "d", "t", "target"
    monkeypatch.setattr(rt, "draw_ray_batch", fake_draw)
    monkeypatch.setattr(RayBatchDataset, "_resident_all",
                        lambda self: (types.SimpleNamespace(shape=(self.n_views, 24, 24, 4)), "cams"))
    return calls


def test_an_epoch_is_one_permutation_with_the_tail_dropped(drawn):
    ds = _dataset().ray_batches(1000, seed=3)
    assert isinstance(ds, RayBatchDataset)
    assert ds.n_pixels == 5 * 24 * 24 == 2880 and len(ds) == 2               # 880 pixels of each permutation are dropped
    for epoch in range(3):
        batches = list(ds)
        assert batches == [("target", ("o", "d", "t"))] * 2
    assert [(c["epoch"], c["first"], c["n"]) for c in drawn] == [(e, f, 1000) for e in range(3) for f in (0, 1000)]
    assert all(c["seed"] == 3 and c["n_samples"] == 8 for c in drawn)
    assert len({c["stream"] for c in drawn}) == len(drawn)                    # every batch has its own jitter stream


def test_steps_per_epoch_continue_through_the_permutation_into_the_next(drawn):
    ds = _dataset().ray_batches(1000, steps_per_epoch=3)
    assert len(ds) == 3
    for _ in range(2):
        assert len(list(ds)) == 3
    # two steps fit a permutation of 2880 pixels: the third step opens the next permutation
    assert [(c["epoch"], c["first"]) for c in drawn] == [(0, 0), (0, 1000), (1, 0), (1, 1000), (2, 0), (2, 1000)]


def test_ranks_draw_disjoint_slices_of_the_same_positions(drawn):
    world = 4
    for r in range(world):
        assert len(list(_dataset(rank=r, world=world).ray_batches(1000, seed=1))) == 2
    per_step = {}
    for c in drawn:
        assert c["n"] == 250 and c["seed"] == 1 and c["epoch"] == 0
        per_step.setdefault(c["first"] // 1000, []).append(c["first"])
    assert per_step == {0: [0, 250, 500, 750], 1: [1000, 1250, 1500, 1750]}
    assert len({c["stream"] for c in drawn}) == len(drawn)                    # the ranks jitter differently
    with pytest.raises(ValueError, match="not divisible"):
        list(_dataset(rank=0, world=3).ray_batches(1000))


def test_a_dataset_beyond_the_device_budget_is_refused_by_name():
    ds = _dataset(device_cache_gb=1e-5).ray_batches(1000)                      # 2880 pixels x 16 B = 46 kB against 10 kB
    with pytest.raises(ValueError, match="device_cache_gb = 1e-05"):
        iter(ds)
    with pytest.raises(ValueError, match="pixels"):
        _dataset().ray_batches(2881)


def test_load_dataset_keeps_its_results(tmp_path):
    from keras_nerf_amd.data.loader import DatasetLoader, RayImageDataset
    from tests.synthetic_scene import write
    root = write(str(tmp_path / "scene"), n=(5, 2, 3))
    out = DatasetLoader(root, white_background=True).load_dataset(2, 24, 24, 2.0, 6.0, 64)
    assert len(out) == 3 and all(type(d) is RayImageDataset for d in out) and [len(d) for d in out] == [2, 1, 1]
    rb = out[0].ray_batches(576)
    assert len(rb) == 5 and rb.n_views == 5
