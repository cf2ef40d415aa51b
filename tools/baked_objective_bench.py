"""Robust losses and ray regularisers on the baked-field optimisers, one GPU, one JSON document (profiles/baked_objective_bench.json
with --out).  Scene and protocol are those of tools/baked_finetune_bench.py and tools/baked_coarse_to_fine_bench.py: the compact
procedural scene at 128 x 128, 40 training views and 4 held out, the MLP trained --train-steps steps, degree 2, termination 1e-4,
white background.
  (a) the gradient launch (accumulate(): the launch and the float64 sums behind it), plain against extended, on the fields baked at
      128^3 and 256^3 with --rays rays: mse + both regularisers, huber alone, distortion alone.  The four optimisers of a lattice take
      turns back to back in one process on the same batch, device events around each call, --timed rounds after --warmup; the gradient
      rows are zeroed outside the timed window.  Median, minimum and maximum per objective and the median's ratio to the plain one.
  (b) held-out PSNR (mean and worst view) after --steps steps: plain fine-tuning of the 256^3 bake; the same with distortion and with
      opacity_entropy at two weights each; and the no-MLP route uniform 64^3 -> 127^3 -> 253^3 of tools/baked_coarse_to_fine_bench.py
      (TV on) with and without both regularisers.  Every run for each of --seeds ray-batch seeds.
The weights are this tool's, not product defaults.  Nothing gates on these numbers; they are reported as they are.

    python tools/baked_objective_bench.py [--train-steps 600] [--steps 300] [--rays 32768] [--out profiles/baked_objective_bench.json]
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
    ap.add_argument("--steps", type=int, default=300, help="ray-batch steps of every run of (b), all stages together")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timed", type=int, default=20, help="timed rounds of (a)")
    ap.add_argument("--rays", type=int, default=32768, help="rays per step")
    ap.add_argument("--lr-sigma", type=float, default=0.3)
    ap.add_argument("--lr-sh", type=float, default=3e-3)
    ap.add_argument("--tv-sigma", type=float, default=1e-5)
    ap.add_argument("--tv-sh", type=float, default=1e-3)
    ap.add_argument("--distortion", default="1e-3,1e-2", help="the two distortion weights of (b)")
    ap.add_argument("--opacity-entropy", default="1e-4,1e-3", help="the two opacity-entropy weights of (b)")
    ap.add_argument("--huber-delta", type=float, default=0.1)
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps of the baked march")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--seeds", default="7,8")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from baked_finetune_bench import HELD, N_TRAIN, WH, write_scene
    from keras_nerf_amd import losses
    from keras_nerf_amd.baked import BakedField
    from keras_nerf_amd.baked_train import fit_coarse_to_fine
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.data.utils import pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene

    degree = 2
    bounds = ((-1.5,) * 3, (1.5,) * 3)
    dist = [float(x) for x in args.distortion.split(",")]
    ent = [float(x) for x in args.opacity_entropy.split(",")]
    seeds = [int(x) for x in args.seeds.split(",")]
    out = {"tool": "baked_objective_bench", "wh": WH, "steps": args.steps, "rays_per_step": args.rays, "lr_sigma": args.lr_sigma,
           "lr_sh": args.lr_sh, "threshold": args.threshold, "sigma_threshold": args.sigma_threshold, "sh_degree": degree,
           "huber_delta": args.huber_delta, "seeds": seeds, "device": torch.cuda.get_device_name(0)}
    V = N_TRAIN + len(HELD)
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=WH, n_views=V, scale=1.6, compact=True)
    c0.close()
    poses = [pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]
    root = tempfile.mkdtemp(prefix="knerf_baked_objective_")
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

    march = dict(white_background=True, termination=args.threshold)
    objectives = {"plain": {},
                  "mse_distortion_entropy": dict(loss="mse", regularizers=losses.RayRegularizers(distortion=dist[0], opacity_entropy=ent[0])),
                  "huber": dict(loss=losses.Huber(args.huber_delta)),
                  "mse_distortion": dict(loss="mse", regularizers=losses.RayRegularizers(distortion=dist[0]))}

    # ---- (a) the gradient launch, plain against extended
    fields = {res: nerf.bake(resolution=res, sh_degree=degree, sigma_threshold=args.sigma_threshold) for res in (128, 256)}
    out["gradient_launch"] = {}
    target, (bo, bd, _) = next(batches(99))
    for res, field in fields.items():
        opts = {name: field.optimizer(args.lr_sigma, args.lr_sh, **march, **kw) for name, kw in objectives.items()}
        ms = {name: [] for name in opts}
        for k in range(args.warmup + args.timed):
            for name, opt in opts.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); opt.accumulate(bo, bd, 2.0, 6.0, target); e1.record(); e1.synchronize()
                opt._grad.zero_()
                if k >= args.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        med = {name: float(np.median(v)) for name, v in ms.items()}
        out["gradient_launch"][f"{res}^3"] = {
            "slots": opts["plain"].n_slots, "rounds": args.timed,
            "ms": {name: {"median": round(med[name], 3), "min": round(min(v), 3), "max": round(max(v), 3),
                          "ratio_to_plain": round(med[name] / med["plain"], 3)} for name, v in ms.items()}}
        del opts
    f256 = fields[256]
    del fields

    # ---- (b) held-out PSNR after --steps steps
    def finetune(seed, **kw):
        opt = f256.optimizer(args.lr_sigma, args.lr_sh, **march, **kw)
        hist = opt.fit(batches(seed), 2.0, 6.0, steps=args.steps)
        entry = {"psnr_held_out": psnr(opt.finish()), "loss_first_last": [float(np.mean(hist["loss"][:10])), float(np.mean(hist["loss"][-10:]))]}
        for key in ("mse", "distortion", "opacity_entropy"):
            if key in hist:
                entry[key + "_first_last"] = [float(np.mean(hist[key][:10])), float(np.mean(hist[key][-10:]))]
        return entry

    runs = [("plain", {})]
    runs += [(f"distortion_{w:g}", dict(regularizers=losses.RayRegularizers(distortion=w))) for w in dist]
    runs += [(f"opacity_entropy_{w:g}", dict(regularizers=losses.RayRegularizers(opacity_entropy=w))) for w in ent]
    out["finetune_256"] = {"psnr_start": psnr(f256), "runs": {name: {f"seed_{s}": finetune(s, **kw) for s in seeds} for name, kw in runs}}
    del f256

    third = args.steps // 3
    stages = [(None, third), (127, third), (253, args.steps - 2 * third)]
    tv = dict(tv_sigma=args.tv_sigma, tv_sh=args.tv_sh)
    both = dict(regularizers=losses.RayRegularizers(distortion=dist[1], opacity_entropy=ent[1]))
    out["uniform_64_127_253"] = {"tv": tv, "regularizers": {"distortion": dist[1], "opacity_entropy": ent[1]}, "runs": {}}
    for name, kw in (("tv_only", {}), ("tv_and_regularizers", both)):
        entry = {}
        for s in seeds:
            start = BakedField.uniform(64, bounds, degree, sigma=0.1, colour=0.5)
            field, hist = fit_coarse_to_fine(start, batches(s), 2.0, 6.0, stages, learning_rate_sigma=args.lr_sigma,
                                             learning_rate_sh=args.lr_sh, **march, **tv, **kw)
            entry[f"seed_{s}"] = {"psnr_held_out": psnr(field), "slots": [st["n_slots"] for st in hist["stages"]],
                                  "loss_first_last": [float(np.mean(hist["loss"][:10])), float(np.mean(hist["loss"][-10:]))]}
            del start, field
        out["uniform_64_127_253"]["runs"][name] = entry
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
