"""Coarse-to-fine optimisation of a baked field with the TV regulariser, one GPU, one JSON document
(profiles/baked_coarse_to_fine_bench.json with --out).  Scene and protocol are those of tools/baked_finetune_bench.py: the compact
procedural scene at 128 x 128, 40 training views and 4 held out, the MLP trained --train-steps steps, degree 2, termination 1e-4,
white background.  Four runs with the same --steps ray-batch steps in total, held-out PSNR (mean and worst view) of each:
  (a) bake at 256^3, fine-tune at 256^3, TV off        DESIGN.md 2.20's baseline, re-measured here
  (b) bake at 128^3, stages 128^3 -> 255^3, TV off     (half of the steps each)
  (c) the same with TV on
  (d) BakedField.uniform, stages 64^3 -> 127^3 -> 253^3, TV on: no bake, the MLP is not used  (a third of the steps each)
and, on (c)'s 255^3 lattice, the milliseconds of the three launches of one regularised step by device events (median over --timed
steps) and of BakedField.resample 128^3 -> 255^3.  The TV weights are this tool's (--tv-sigma, --tv-sh), not product defaults.
Nothing gates on these numbers.

    python tools/baked_coarse_to_fine_bench.py [--train-steps 600] [--steps 300] [--rays 32768] [--out profiles/baked_coarse_to_fine_bench.json]
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
    ap.add_argument("--train-steps", type=int, default=600)
    ap.add_argument("--steps", type=int, default=300, help="ray-batch steps of every run, all stages together")
    ap.add_argument("--timed", type=int, default=20, help="further steps timed launch by launch")
    ap.add_argument("--rays", type=int, default=32768, help="rays per step")
    ap.add_argument("--lr-sigma", type=float, default=0.3)
    ap.add_argument("--lr-sh", type=float, default=3e-3)
    ap.add_argument("--tv-sigma", type=float, default=1e-5)
    ap.add_argument("--tv-sh", type=float, default=1e-3)
    ap.add_argument("--tv-epsilon", type=float, default=1e-6)
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps of the baked march")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--tv-sweep", default="", help='further weight pairs for run (c), "tv_sigma,tv_sh;tv_sigma,tv_sh": how --tv-sigma / --tv-sh were chosen')
    ap.add_argument("--runs", default="a,b,c,d")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from baked_finetune_bench import HELD, N_TRAIN, WH, write_scene
    from keras_nerf_amd.baked import BakedField, n_coefficients
    from keras_nerf_amd.baked_train import fit_coarse_to_fine
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.data.utils import pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene

    degree = 2
    bounds = ((-1.5,) * 3, (1.5,) * 3)
    tv = dict(tv_sigma=args.tv_sigma, tv_sh=args.tv_sh, tv_epsilon=args.tv_epsilon)
    out = {"tool": "baked_coarse_to_fine_bench", "wh": WH, "steps": args.steps, "rays_per_step": args.rays, "lr_sigma": args.lr_sigma,
           "lr_sh": args.lr_sh, "tv": tv, "threshold": args.threshold, "sigma_threshold": args.sigma_threshold, "sh_degree": degree,
           "device": torch.cuda.get_device_name(0)}
    V = N_TRAIN + len(HELD)
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=WH, n_views=V, scale=1.6, compact=True)
    c0.close()
    poses = [pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]
    root = tempfile.mkdtemp(prefix="knerf_baked_c2f_")
    train_views = torch.as_tensor(write_scene(root, img.cpu().numpy(), poses), device="cuda")
    train_ds, _, _ = DatasetLoader(root, white_background=True).load_dataset(2, WH, WH, 2.0, 6.0, 64)

    nerf = NeRF(seed=0)
    nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=2, image_height=WH, image_width=WH, ray_chunks=4096, white_background=True)
    order = np.random.default_rng(5).integers(0, N_TRAIN, (args.train_steps, 2))
    t0 = time.time()
    for s in range(args.train_steps):
        idx = train_views[torch.as_tensor(order[s], device="cuda")]
        nerf.train_step((img[idx], (o[idx], d[idx], t[idx])), with_metrics=False)
    nerf._ctx.poll_nonfinite(wait=True)
    out["train"] = f"compact procedural scene, {WH}x{WH}, batch 2, {args.train_steps} steps on {N_TRAIN} views ({time.time() - t0:.1f} s)"

    held = list(HELD)
    truth = [img[i].reshape(-1, 3) for i in held]
    flat = [(o[i].reshape(-1, 3), d[i].reshape(-1, 3)) for i in held]

    def psnr(field):
        imgs = [field.render(a, b, 2.0, 6.0, white_background=True, termination=args.threshold, outputs="image")["image"] for a, b in flat]
        v = [float(-10 * np.log10(max(float(((a - b) ** 2).mean()), 1e-20))) for a, b in zip(imgs, truth)]
        return {"min": round(min(v), 2), "mean": round(float(np.mean(v)), 2)}

    def batches(seed):
        """ray batches without end: one epoch of the dataset after the other"""
        while True:
            n = 0
            for b in train_ds.ray_batches(args.rays, seed=seed):
                n += 1
                yield b
            if not n:
                return
            seed += 1000

    def run(start, stages, regularised, tv=tv):
        kw = dict(learning_rate_sigma=args.lr_sigma, learning_rate_sh=args.lr_sh, white_background=True, termination=args.threshold)
        torch.cuda.synchronize(); t0 = time.time()
        field, hist = fit_coarse_to_fine(start, batches(7), 2.0, 6.0, stages, **kw, **(tv if regularised else {}))
        torch.cuda.synchronize()
        entry = {"stages": [{"resolution": list(s["resolution"]), "steps": s["steps"], "slots": s["n_slots"]} for s in hist["stages"]],
                 "tv": bool(regularised), "fit_seconds": round(time.time() - t0, 2),
                 "loss_first_last": [float(np.mean(hist["loss"][:10])), float(np.mean(hist["loss"][-10:]))], "psnr_held_out": psnr(field)}
        if regularised:
            entry["tv_sigma_first_last"] = [hist["tv_sigma"][0], hist["tv_sigma"][-1]]
            entry["tv_sh_first_last"] = [hist["tv_sh"][0], hist["tv_sh"][-1]]
        return field, entry

    wanted = [r for r in args.runs.split(",") if r]
    half, third = args.steps // 2, args.steps // 3
    out["runs"] = {}
    if "a" in wanted:
        f256 = nerf.bake(resolution=256, sh_degree=degree, sigma_threshold=args.sigma_threshold)
        base = psnr(f256)
        _, e = run(f256, [(None, args.steps)], False)
        out["runs"]["a"] = {"start": "bake at 256^3", "psnr_start": base, **e}
        del f256
    done_c = None
    if "b" in wanted or "c" in wanted:
        f128 = nerf.bake(resolution=128, sh_degree=degree, sigma_threshold=args.sigma_threshold)
        base = psnr(f128)
        for name, reg in (("b", False), ("c", True)):
            if name in wanted:
                field, e = run(f128, [(None, half), (255, args.steps - half)], reg)
                out["runs"][name] = {"start": "bake at 128^3", "psnr_start": base, **e}
                if reg:
                    done_c = field
        for pair in (p for p in args.tv_sweep.split(";") if p):
            ts, tc = (float(x) for x in pair.split(","))
            _, e = run(f128, [(None, half), (255, args.steps - half)], True, dict(tv_sigma=ts, tv_sh=tc, tv_epsilon=args.tv_epsilon))
            out.setdefault("c_sweep", {})[pair] = {k: e[k] for k in ("psnr_held_out", "loss_first_last", "tv_sigma_first_last", "tv_sh_first_last")}
        # BakedField.resample 128^3 -> 255^3 (the launch, the fresh table and the new occupancy bits), after one warm-up
        f128.resample(255)
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f128.resample(255); e1.record(); e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        rb = 64
        out["resample_128_to_255"] = {"ms": round(float(np.median(ms)), 3),
                                      "gigabytes_per_second_written": round(255 ** 3 * rb / (float(np.median(ms)) * 1e-3) / 1e9, 1)}
        del f128
    if "d" in wanted:
        start = BakedField.uniform(64, bounds, degree, sigma=0.1, colour=0.5)
        _, e = run(start, [(None, third), (127, third), (253, args.steps - 2 * third)], True)
        out["runs"]["d"] = {"start": "BakedField.uniform(64, sigma 0.1, colour 0.5), no bake", **e}
        del start
    if done_c is not None:
        # one regularised step on (c)'s lattice, launch by launch
        W = 1 + 3 * n_coefficients(degree)
        opt = done_c.optimizer(args.lr_sigma, args.lr_sh, white_background=True, termination=args.threshold, **tv)
        ms = {"gradient_launch": [], "tv_launch": [], "adam_launch": []}
        for k, (target, (bo, bd, _)) in enumerate(batches(99)):
            if k >= args.timed + 2:
                break
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(); opt.accumulate(bo, bd, 2.0, 6.0, target); e[1].record(); opt.regularize(); e[2].record(); opt.apply(); e[3].record()
            e[3].synchronize()
            if k >= 2:
                for j, key in enumerate(ms):
                    ms[key].append(e[j].elapsed_time(e[j + 1]))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out["step_on_255"] = {"slots": opt.n_slots, "lattice_points": 255 ** 3, "ms": {k: round(v, 3) for k, v in med.items()},
                              # the least the TV launch must move: master read, gradient read and written, the two sums written, point_of read
                              "tv_gigabytes_per_second_at_least": round(opt.n_slots * (W * 12 + 12) / (med["tv_launch"] * 1e-3) / 1e9, 1),
                              "adam_gigabytes_per_second": round(opt.n_slots * (W * 4 * 7 + 64) / (med["adam_launch"] * 1e-3) / 1e9, 1)}
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
