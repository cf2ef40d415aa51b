"""Empty-space skipping in TRAINING (option occupancy_train, OccupancyGridUpdater), one GPU, one JSON line.

Step time: the cfg2 shape (128 x 128, batch 2, ray_chunks 4096, coarse 64 + fine 128) on the compact procedural scene
(tests/procedural_scene.py, density exactly 0 outside the objects), trained for --train-steps dense steps to a steady state; then grids
from the trained field (OccupancyGridUpdater.update: density EMA on a --grid^3 lattice), and steps alternating between dense and grid +
occupancy_train (device events around each train_step, --warmup steps of each first, median ms per step); the live fractions of each
net's training samples (occupancy_train_stats); the time of one grid update.
Quality: the same --quality-steps training run twice from the same initial weights, dense and with OccupancyGridUpdater (warm-up
--quality-warmup, an update every 16 steps); fine PSNR on --held-out poses that neither run trains on.

    python tools/occupancy_train_bench.py [--train-steps 600] [--steps 40] [--warmup 5] [--grid 128] [--quality-steps 1500]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=600)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--quality-steps", type=int, default=1500)
    ap.add_argument("--quality-warmup", type=int, default=256)
    ap.add_argument("--held-out", type=int, default=4)
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd.model.nerf.callback import OccupancyGridUpdater
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene

    wh, B, R, V = 128, 2, 4096, 40
    out = {"tool": "occupancy_train_bench", "wh": wh, "batch": B, "ray_chunks": R, "n_coarse": 64, "n_fine": 128, "grid": args.grid,
           "train_steps": args.train_steps, "steps": args.steps}
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=wh, n_views=V, scale=1.6, compact=True)
    c0.close()
    n_train = V - args.held_out

    def model():
        m = NeRF(seed=0)
        m.compile({"learning_rate": 5e-4}, "mse", batch_size=B, image_height=wh, image_width=wh, ray_chunks=R, white_background=True)
        return m

    def batch(order, s):
        idx = torch.as_tensor(order[s], device="cuda")
        return img[idx], (o[idx], d[idx], t[idx])

    # ---- step time
    nerf = model()
    order = np.random.default_rng(5).integers(0, n_train, (args.train_steps + 2 * (args.steps + args.warmup), B))
    t0 = time.time()
    for s in range(args.train_steps):
        nerf.train_step(batch(order, s), with_metrics=False)
    nerf._ctx.poll_nonfinite(wait=True)
    out["train_s"] = round(time.time() - t0, 1)
    upd = OccupancyGridUpdater(update_every=1, warmup_steps=0, resolution=args.grid)
    upd.set_model(nerf)
    upd.update()                                 # allocations and the first grid
    torch.cuda.synchronize()
    ms_upd = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); upd.update(); b.record(); b.synchronize()
        ms_upd.append(a.elapsed_time(b))
    out["grid_update_ms"] = round(float(np.median(ms_upd)), 3)
    ms = {"dense": [], "occ": []}
    s = args.train_steps
    nerf.occupancy_train_stats(reset=True)
    for i in range(2 * (args.steps + args.warmup)):
        mode = "dense" if i % 2 == 0 else "occ"
        nerf.set_occupancy_training(mode == "occ")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        nerf.train_step(batch(order, s), with_metrics=False)
        b.record(); b.synchronize()
        s += 1
        if i >= 2 * args.warmup:
            ms[mode].append(a.elapsed_time(b))
    st = nerf.occupancy_train_stats()
    out["dense_ms"] = round(float(np.median(ms["dense"])), 3)
    out["occ_ms"] = round(float(np.median(ms["occ"])), 3)
    out["speedup"] = round(out["dense_ms"] / out["occ_ms"], 3)
    out["live"] = {k: round(v[0] / max(v[1], 1), 4) for k, v in st.items()}
    nerf._ctx.close()

    # ---- quality
    order = np.random.default_rng(6).integers(0, n_train, (args.quality_steps, B))
    u = torch.rand((B, wh, wh, 128), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    psnr = {}
    for name in ("dense", "grid"):
        m = model()
        cb = OccupancyGridUpdater(update_every=16, warmup_steps=args.quality_warmup, resolution=args.grid) if name == "grid" else None
        if cb:
            cb.set_model(m)
        t0 = time.time()
        for s in range(args.quality_steps):
            m.train_step(batch(order, s), with_metrics=False)
            if cb:
                cb.on_train_batch_end(s, {})
        m._ctx.poll_nonfinite(wait=True)
        out[f"quality_{name}_train_s"] = round(time.time() - t0, 1)
        if cb:
            st = m.occupancy_train_stats()
            out["quality_live"] = {k: round(v[0] / max(v[1], 1), 4) for k, v in st.items()}
        vals = []
        for v0 in range(n_train, V, B):
            idx = torch.arange(v0, min(v0 + B, V), device="cuda")
            if len(idx) < B:
                break
            f = m.predict_and_render_images((o[idx], d[idx], t[idx]), u=u, outputs=("image",))[1]["image"]
            vals.append(-10 * np.log10(max(float(((f - img[idx]) ** 2).mean()), 1e-20)))
        psnr[name] = round(float(np.mean(vals)), 3)
        m._ctx.close()
    out["quality_steps"] = args.quality_steps
    out["quality_warmup"] = args.quality_warmup
    out["psnr_held_out_dense"], out["psnr_held_out_grid"] = psnr["dense"], psnr["grid"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
