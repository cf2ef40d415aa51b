"""Per-ray backgrounds and the opacity loss on the baked-field optimisers, one GPU, one JSON document (profiles/baked_rgba_bench.json
with --out).  Scene and protocol are those of tools/baked_objective_bench.py: the compact procedural scene at 128 x 128, 40 training
views and 4 held out, the MLP trained --train-steps steps, degree 2, termination 1e-4.  The photographs are RGBA here: their alpha is
the scene's own sum of weights, their colour is stored over white as ImageLoader(white_background=True) stores it.
  (a) the gradient launch (accumulate(): the launch and the float64 sums behind it), the rgba launch against the _ext launch of the
      same run, on the fields baked at 128^3 and 256^3 with --rays rays, under mse + distortion + opacity entropy: "ext" (white flag,
      [n,3] targets), "rgba_fixed" (one [n,3] background tensor passed per call, [n,4] targets, opacity loss) and "rgba_random" (the
      same with background="random": the draw of torch.rand is inside the timed window).  The optimisers take turns back to back on
      the same batch, device events around each call, --timed rounds after --warmup; the gradient rows are zeroed outside the timed
      window.  Median, minimum and maximum and the median's ratio to "ext".  The yardstick is the _ext launch; there is no pass mark.
  (b) held-out PSNR (mean and worst view, rendered over white) and the mean rendered opacity over the held-out pixels whose alpha is 0,
      after --steps steps: BakedField.uniform 64^3 -> 127^3 -> 253^3 (TV on) and the fine-tuned 256^3 bake, each plain (white flag,
      [n,3] targets: what the optimisers did before) and with background="random" at two opacity_loss weights, for each of --seeds
      ray-batch seeds.
The weights are this tool's, not product defaults.  Nothing gates on these numbers; they are reported as they are.

    python tools/baked_rgba_bench.py [--train-steps 600] [--steps 300] [--rays 32768] [--out profiles/baked_rgba_bench.json]
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


def scene_alpha(o, d, scale, compact):
    """the procedural scene's own opacity per pixel: the sum of weights of tests/procedural_scene.make_scene's march (512 samples, fp64)"""
    import torch
    from tests.procedural_scene import field
    tt = torch.linspace(2.0, 6.0, 512, device="cuda", dtype=torch.float64)
    delta = torch.cat([tt[1:] - tt[:-1], tt.new_full((1,), 1e-10)])
    out = []
    for v in range(o.shape[0]):
        p = o[v].double()[..., None, :] + d[v].double()[..., None, :] * tt[:, None]
        sg, _ = field(p, scale, compact)
        a = 1.0 - torch.exp(-sg * delta)
        T = torch.cumprod(torch.cat([torch.ones_like(a[..., :1]), 1.0 - a[..., :-1] + 1e-10], -1), -1)
        out.append((a * T).sum(-1).clamp(0, 1).float())
    return torch.stack(out)


def write_rgba_scene(root, img, alpha, poses, held):
    """transforms_{train,val,test}.json + RGBA PNGs with straight colour (img is the colour over white: rgb = (img - (1 - alpha)) /
    alpha) and the scene's alpha, so that ImageLoader(white_background=True) gives img back up to the 8 bits of the file"""
    import numpy as np
    from PIL import Image
    from tests.procedural_scene import FOV
    views = range(len(poses))
    split = {"train": [i for i in views if i not in held], "val": list(held), "test": list(held)}
    for subset, idx in split.items():
        os.makedirs(os.path.join(root, subset), exist_ok=True)
        frames = []
        for k, i in enumerate(idx):
            a = alpha[i][..., None]
            rgb = np.where(a > 0, (img[i] - (1.0 - a)) / np.maximum(a, 1e-6), 1.0).clip(0, 1)
            rgba = np.concatenate([rgb, a], -1)
            Image.fromarray((rgba * 255 + 0.5).astype(np.uint8), "RGBA").save(os.path.join(root, subset, f"r_{k}.png"))
            frames.append({"file_path": f"./{subset}/r_{k}", "transform_matrix": np.asarray(poses[i]).tolist()})
        json.dump({"camera_angle_x": FOV, "frames": frames}, open(os.path.join(root, f"transforms_{subset}.json"), "w"))
    return split["train"]


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
    ap.add_argument("--opacity-loss", default="1e-3,1e-2", help="the two opacity_loss weights of (b); (a) uses the first")
    ap.add_argument("--distortion", type=float, default=1e-3, help="the distortion weight of (a)")
    ap.add_argument("--opacity-entropy", type=float, default=1e-4, help="the opacity-entropy weight of (a)")
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps of the baked march")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--seeds", default="7,8")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from baked_finetune_bench import HELD, N_TRAIN, WH
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
    weights = [float(x) for x in args.opacity_loss.split(",")]
    seeds = [int(x) for x in args.seeds.split(",")]
    out = {"tool": "baked_rgba_bench", "wh": WH, "steps": args.steps, "rays_per_step": args.rays, "lr_sigma": args.lr_sigma,
           "lr_sh": args.lr_sh, "threshold": args.threshold, "sigma_threshold": args.sigma_threshold, "sh_degree": degree,
           "opacity_loss": weights, "seeds": seeds, "device": torch.cuda.get_device_name(0)}

    def note(text):
        print(f"[{time.strftime('%H:%M:%S')}] {text}", file=sys.stderr, flush=True)

    V = N_TRAIN + len(HELD)
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=WH, n_views=V, scale=1.6, compact=True)
    c0.close()
    alpha = scene_alpha(o, d, 1.6, True)
    poses = [pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]
    root = tempfile.mkdtemp(prefix="knerf_baked_rgba_")
    train_views = torch.as_tensor(write_rgba_scene(root, img.cpu().numpy(), alpha.cpu().numpy(), poses, HELD), device="cuda")
    train_ds, _, _ = DatasetLoader(root, white_background=True).load_dataset(2, WH, WH, 2.0, 6.0, 64)
    out["alpha"] = {"empty_share_train": round(float((alpha[train_views] == 0).float().mean()), 4),
                    "interior_share_train": round(float(((alpha[train_views] > 0) & (alpha[train_views] < 1)).float().mean()), 4)}

    nerf = NeRF(seed=0)
    nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=2, image_height=WH, image_width=WH, ray_chunks=4096, white_background=True)
    order = np.random.default_rng(5).integers(0, N_TRAIN, (args.train_steps, 2))
    t0 = time.time()
    for s in range(args.train_steps):
        idx = train_views[torch.as_tensor(order[s], device="cuda")]
        nerf.train_step((img[idx], (o[idx], d[idx], t[idx])), with_metrics=False)
    nerf._ctx.poll_nonfinite(wait=True)
    out["train"] = f"compact procedural scene, {WH}x{WH}, batch 2, {args.train_steps} steps on {N_TRAIN} views ({time.time() - t0:.1f} s)"
    note(out["train"])

    held = list(HELD)
    truth = [img[i].reshape(-1, 3) for i in held]
    empty = [alpha[i].reshape(-1) == 0 for i in held]
    flat = [(o[i].reshape(-1, 3), d[i].reshape(-1, 3)) for i in held]

    def quality(field):
        """held-out PSNR over white, and the mean rendered opacity where the photographs are empty"""
        res = [field.render(a, b, 2.0, 6.0, white_background=True, termination=args.threshold, outputs=("image", "opacity")) for a, b in flat]
        v = [float(-10 * np.log10(max(float(((r["image"] - b) ** 2).mean()), 1e-20))) for r, b in zip(res, truth)]
        floor = torch.cat([r["opacity"][m] for r, m in zip(res, empty)])
        return {"psnr_min": round(min(v), 2), "psnr_mean": round(float(np.mean(v)), 2), "opacity_where_alpha_0": float(floor.mean()),
                "pixels_alpha_0": int(floor.numel())}

    def batches(seed, with_alpha):
        """ray batches without end: one epoch of the dataset after the other"""
        while True:
            n = 0
            for b in train_ds.ray_batches(args.rays, seed=seed, alpha=with_alpha):
                n += 1
                yield b
            if not n:
                return
            seed += 1000

    march = dict(termination=args.threshold)
    plain = dict(white_background=True)
    rgba = lambda w: dict(background="random", opacity_loss=w, target_background="white")

    # ---- (a) the gradient launch, rgba against _ext
    regs = dict(loss="mse", regularizers=losses.RayRegularizers(distortion=args.distortion, opacity_entropy=args.opacity_entropy))
    fields = {res: nerf.bake(resolution=res, sh_degree=degree, sigma_threshold=args.sigma_threshold) for res in (128, 256)}
    out["gradient_launch"] = {"objective": {"distortion": args.distortion, "opacity_entropy": args.opacity_entropy, "opacity_loss": weights[0]}}
    target4, (bo, bd, _) = next(batches(99, True))
    target3 = target4[:, :3].contiguous()
    fixed = torch.rand((target4.shape[0], 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    for res, field in fields.items():
        opts = {"ext": (field.optimizer(args.lr_sigma, args.lr_sh, **march, **plain, **regs), target3, {}),
                "rgba_fixed": (field.optimizer(args.lr_sigma, args.lr_sh, **march, opacity_loss=weights[0], target_background="white", **regs),
                               target4, dict(background=fixed)),
                "rgba_random": (field.optimizer(args.lr_sigma, args.lr_sh, **march, **rgba(weights[0]), **regs), target4, {})}
        ms = {name: [] for name in opts}
        for k in range(args.warmup + args.timed):
            for name, (opt, tg, extra) in opts.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); opt.accumulate(bo, bd, 2.0, 6.0, tg, **extra); e1.record(); e1.synchronize()
                opt._grad.zero_()
                if k >= args.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        med = {name: float(np.median(v)) for name, v in ms.items()}
        out["gradient_launch"][f"{res}^3"] = {
            "slots": opts["ext"][0].n_slots, "rounds": args.timed,
            "ms": {name: {"median": round(med[name], 3), "min": round(min(v), 3), "max": round(max(v), 3),
                          "ratio_to_ext": round(med[name] / med["ext"], 3)} for name, v in ms.items()}}
        note(f"(a) {res}^3: " + ", ".join(f"{k} {v:.3f} ms" for k, v in med.items()))
        del opts
    f256 = fields[256]
    del fields

    def save():
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")

    # ---- (b) held-out PSNR and the opacity of empty pixels after --steps steps
    runs = [("plain", plain, False)] + [(f"random_opacity_{w:g}", rgba(w), True) for w in weights]

    def finetune(seed, kw, with_alpha):
        opt = f256.optimizer(args.lr_sigma, args.lr_sh, **march, **kw)
        hist = opt.fit(batches(seed, with_alpha), 2.0, 6.0, steps=args.steps)
        entry = {**quality(opt.finish()), "loss_first_last": [float(np.mean(hist["loss"][:10])), float(np.mean(hist["loss"][-10:]))]}
        if "opacity" in hist:
            entry["opacity_term_first_last"] = [float(np.mean(hist["opacity"][:10])), float(np.mean(hist["opacity"][-10:]))]
        return entry

    out["finetune_256"] = {"start": quality(f256), "runs": {}}
    for name, kw, with_alpha in runs:
        out["finetune_256"]["runs"][name] = {}
        for s in seeds:
            out["finetune_256"]["runs"][name][f"seed_{s}"] = finetune(s, kw, with_alpha)
            note(f"(b) fine-tune 256^3 {name} seed {s}: {out['finetune_256']['runs'][name][f'seed_{s}']}")
            save()
    del f256

    third = args.steps // 3
    stages = [(None, third), (127, third), (253, args.steps - 2 * third)]
    tv = dict(tv_sigma=args.tv_sigma, tv_sh=args.tv_sh)
    out["uniform_64_127_253"] = {"tv": tv, "runs": {}}
    for name, kw, with_alpha in runs:
        entry = {}
        for s in seeds:
            start = BakedField.uniform(64, bounds, degree, sigma=0.1, colour=0.5)
            field, hist = fit_coarse_to_fine(start, batches(s, with_alpha), 2.0, 6.0, stages, learning_rate_sigma=args.lr_sigma,
                                             learning_rate_sh=args.lr_sh, **march, **tv, **kw)
            entry[f"seed_{s}"] = {**quality(field), "slots": [st["n_slots"] for st in hist["stages"]],
                                  "loss_first_last": [float(np.mean(hist["loss"][:10])), float(np.mean(hist["loss"][-10:]))]}
            note(f"(b) uniform route {name} seed {s}: {entry[f'seed_{s}']}")
            del start, field
        out["uniform_64_127_253"]["runs"][name] = entry
        save()
    print(json.dumps(out))
    save()


if __name__ == "__main__":
    main()
