"""Growing a baked field on its brick storage against the dense path, one GPU, one JSON document
(profiles/baked_bricks_grow_bench.json with --out).  Scene and protocol are those of tools/baked_coarse_to_fine_bench.py: the compact
procedural scene at 128 x 128, 40 training views and 4 held out, the MLP trained --train-steps steps (it is used for the bakes of (a)
and (b) only), degree 2, termination 1e-4, white background.  Times are device events, medians over --repeat, the two sides alternating
in one process; memory is torch.cuda.max_memory_allocated above what was allocated when the measured call began.
  (a) resample_bricks against to_dense().resample().compact() at 128^3 -> 255^3 and 256^3 -> 511^3: milliseconds and peak bytes
  (b) knerf_baked_bricks_train_tv against knerf_baked_train_tv on the same 255^3 field, one launch each
  (c) BakedField.uniform(64) -> 127^3 -> 253^3 through baked_train.fit_coarse_to_fine, threshold 0: run (d) of DESIGN.md 2.21 as it stands
  (d) the same start compacted, through fit_coarse_to_fine_bricks, for every "sigma_threshold,prune_every" of --sweep, at --steps and at
      --more-steps: held-out PSNR, bricks / records / slots per stage, the prunes, peak memory
Nothing gates on these numbers; every figure is reported as measured.

    python tools/baked_bricks_grow_bench.py [--parts a,b,c,d] [--steps 300] [--more-steps 900] [--out profiles/baked_bricks_grow_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c,d")
    ap.add_argument("--train-steps", type=int, default=600)
    ap.add_argument("--steps", type=int, default=300, help="ray-batch steps of (c) and (d), all stages together")
    ap.add_argument("--more-steps", type=int, default=900, help="the larger step budget of (d); 0: none")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--rays", type=int, default=32768, help="rays per step")
    ap.add_argument("--lr-sigma", type=float, default=0.3)
    ap.add_argument("--lr-sh", type=float, default=3e-3)
    ap.add_argument("--tv-sigma", type=float, default=1e-5)
    ap.add_argument("--tv-sh", type=float, default=1e-3)
    ap.add_argument("--tv-epsilon", type=float, default=1e-6)
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps of the baked march")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--sweep", default="0,0;0.5,25;2,25", help='"sigma_threshold,prune_every" pairs of (d); prune_every 0: no prune')
    ap.add_argument("--brick", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from baked_finetune_bench import HELD, N_TRAIN, WH, write_scene
    from keras_nerf_amd.baked import BakedField
    from keras_nerf_amd.baked_bricks_grow import fit_coarse_to_fine_bricks, grid_trainer, resample_bricks
    from keras_nerf_amd.baked_train import fit_coarse_to_fine
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.data.utils import pose_spherical
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene

    parts = [p for p in args.parts.split(",") if p]
    degree, b = 2, args.brick
    bounds = ((-1.5,) * 3, (1.5,) * 3)
    tv = dict(tv_sigma=args.tv_sigma, tv_sh=args.tv_sh, tv_epsilon=args.tv_epsilon)
    out = {"tool": "baked_bricks_grow_bench", "wh": WH, "steps": args.steps, "more_steps": args.more_steps, "rays_per_step": args.rays,
           "lr_sigma": args.lr_sigma, "lr_sh": args.lr_sh, "tv": tv, "threshold": args.threshold, "sigma_threshold_of_the_bakes": args.sigma_threshold,
           "sh_degree": degree, "brick": b, "repeat": args.repeat, "device": torch.cuda.get_device_name(0)}
    V = N_TRAIN + len(HELD)
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=WH, n_views=V, scale=1.6, compact=True)
    c0.close()
    poses = [pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]
    root = tempfile.mkdtemp(prefix="knerf_baked_bricks_grow_")
    train_views = torch.as_tensor(write_scene(root, img.cpu().numpy(), poses), device="cuda")
    train_ds, _, _ = DatasetLoader(root, white_background=True).load_dataset(2, WH, WH, 2.0, 6.0, 64)
    held = list(HELD)
    truth = [img[i].reshape(-1, 3) for i in held]
    flat = [(o[i].reshape(-1, 3), d[i].reshape(-1, 3)) for i in held]

    def psnr(field):
        imgs = [field.render(a, c, 2.0, 6.0, white_background=True, termination=args.threshold, outputs="image")["image"] for a, c in flat]
        v = [float(-10 * np.log10(max(float(((a - c) ** 2).mean()), 1e-20))) for a, c in zip(imgs, truth)]
        return {"min": round(min(v), 2), "mean": round(float(np.mean(v)), 2)}

    def batches(seed):
        """ray batches without end: one epoch of the dataset after the other"""
        while True:
            n = 0
            for batch in train_ds.ray_batches(args.rays, seed=seed):
                n += 1
                yield batch
            if not n:
                return
            seed += 1000

    def measured(call):
        """(milliseconds by device events, peak bytes above the start, the call's result)"""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); result = call(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - start, result

    def alternate(sides):
        """every side --repeat times after one warm-up each, alternating; {name: {"ms": median, "peak_bytes": median}}"""
        got = {name: [] for name in sides}
        for k in range(args.repeat + 1):
            for name, call in sides.items():
                ms, peak, result = measured(call)
                del result
                if k:
                    got[name].append((ms, peak))
        return {name: {"ms": round(float(np.median([v[0] for v in vs])), 3), "peak_bytes": int(np.median([v[1] for v in vs]))}
                for name, vs in got.items()}

    if "a" in parts or "b" in parts:
        from keras_nerf_amd.model.nerf.nerf import NeRF
        nerf = NeRF(seed=0)
        nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=2, image_height=WH, image_width=WH, ray_chunks=4096, white_background=True)
        order = np.random.default_rng(5).integers(0, N_TRAIN, (args.train_steps, 2))
        t0 = time.time()
        for s in range(args.train_steps):
            idx = train_views[torch.as_tensor(order[s], device="cuda")]
            nerf.train_step((img[idx], (o[idx], d[idx], t[idx])), with_metrics=False)
        nerf._ctx.poll_nonfinite(wait=True)
        out["train"] = f"compact procedural scene, {WH}x{WH}, batch 2, {args.train_steps} steps on {N_TRAIN} views ({time.time() - t0:.1f} s)"
        out["resample"] = {}
        for r0, r1 in ((128, 255), (256, 511)):
            bricks = nerf.bake(resolution=r0, sh_degree=degree, sigma_threshold=args.sigma_threshold, bricks=b)
            entry = alternate({"bricks": lambda: resample_bricks(bricks, r1),
                               "dense": lambda: bricks.to_dense().resample(r1).compact(b)})
            done = resample_bricks(bricks, r1)
            entry.update(source_bricks=bricks.n_bricks, source_bytes=bricks.nbytes, result_bricks=done.n_bricks, result_bytes=done.nbytes,
                         dense_destination_table_bytes=r1 ** 3 * 64, occupied_cells=round(float(done.occupied.float().mean()), 4))
            out["resample"][f"{r0}_to_{r1}"] = entry
            if r1 == 255 and "b" in parts:
                # one TV launch on the same 255^3 field, both storages, both re-measured here
                kw = dict(white_background=True, termination=args.threshold, **tv)
                sparse = grid_trainer(done, args.lr_sigma, args.lr_sh, **kw)
                dense = done.to_dense().optimizer(args.lr_sigma, args.lr_sh, **kw)
                entry = alternate({"bricks": sparse.regularize, "dense": dense.regularize})
                entry.update(slots=sparse.n_slots, dense_slots=dense.n_slots, records=sparse.counts()["n_records"], lattice_points=r1 ** 3)
                out["tv_launch_on_255"] = entry
                del sparse, dense
            del bricks, done
        del nerf

    def fit(run, start, stages, **kw):
        common = dict(learning_rate_sigma=args.lr_sigma, learning_rate_sh=args.lr_sh, white_background=True, termination=args.threshold, **tv)
        t0 = time.time()
        ms, peak, (field, hist) = measured(lambda: run(start, batches(7), 2.0, 6.0, stages, **common, **kw))
        keys = ("n_bricks", "n_records", "n_slots")
        return {"stages": [{"resolution": list(s["resolution"]), "steps": s["steps"], **{k: s[k] for k in keys if k in s},
                            **({"prunes": [[p["before"]["n_slots"], p["after"]["n_slots"]] for p in s["prunes"]]} if "prunes" in s else {})}
                           for s in hist["stages"]],
                "fit_seconds": round(time.time() - t0, 2), "peak_bytes": int(peak),
                "loss_first_last": [float(np.mean(hist["loss"][:10])), float(np.mean(hist["loss"][-10:]))], "psnr_held_out": psnr(field)}

    def stages(steps):
        third = steps // 3
        return [(None, third), (127, third), (253, steps - 2 * third)]

    if "c" in parts:
        start = BakedField.uniform(64, bounds, degree, sigma=0.1, colour=0.5)
        out["dense_uniform_64"] = {"start": "BakedField.uniform(64, sigma 0.1, colour 0.5), dense, threshold 0",
                                   **fit(fit_coarse_to_fine, start, stages(args.steps))}
        del start
    if "d" in parts:
        start = BakedField.uniform(64, bounds, degree, sigma=0.1, colour=0.5).compact(b)
        out["bricks_uniform_64"] = {}
        for steps in [args.steps] + ([args.more_steps] if args.more_steps else []):
            for pair in (p for p in args.sweep.split(";") if p):
                thr, every = (float(x) for x in pair.split(","))
                entry = fit(fit_coarse_to_fine_bricks, start, stages(steps), sigma_threshold=thr, prune_every=int(every) or None)
                out["bricks_uniform_64"][f"steps {steps}, sigma_threshold {thr:g}, prune_every {int(every)}"] = entry
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
