"""Fine-tuning a baked field on the photographs, one GPU, one JSON document (profiles/baked_finetune_bench.json with --out):
  - the compact procedural scene (tests/procedural_scene.py) at 128 x 128 written as a nerf_synthetic-layout directory: 40 training
    views and 4 held out; the MLP trained on the training views as tools/baked_bench.py trains it (--train-steps steps, batch 2);
  - NeRF.bake at 128^3 and 256^3, degree 2, then BakedField.optimizer(...).fit on train.ray_batches(--rays) for --steps steps;
  - PSNR on the held-out views against the ground-truth images: the MLP, the baked field, the fine-tuned field (after finish());
  - milliseconds per train_step, split into its two launches by device events (median over --timed steps after the fit), and the
    atomic bytes the gradient launch adds per second: every fetched sample adds 8 corner rows of 1 + 3 K floats (samples whose
    gradient is exactly zero add nothing, so the figure is an upper bound), against the chip's rate of about 1.3 TB/s.
Nothing gates on these numbers.

    python tools/baked_finetune_bench.py [--train-steps 600] [--steps 300] [--rays 32768] [--out profiles/baked_finetune_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WH, N_TRAIN, HELD = 128, 40, (5, 16, 27, 38)


def write_scene(root, img, poses):
    """transforms_{train,val,test}.json + RGBA PNGs (val = test = the held-out views)"""
    import numpy as np
    from PIL import Image
    from tests.procedural_scene import FOV
    views = range(len(poses))
    split = {"train": [i for i in views if i not in HELD], "val": list(HELD), "test": list(HELD)}
    for subset, idx in split.items():
        os.makedirs(os.path.join(root, subset), exist_ok=True)
        frames = []
        for k, i in enumerate(idx):
            rgba = np.concatenate([img[i], np.ones_like(img[i][..., :1])], -1)
            Image.fromarray((rgba * 255 + 0.5).astype(np.uint8), "RGBA").save(os.path.join(root, subset, f"r_{k}.png"))
            frames.append({"file_path": f"./{subset}/r_{k}", "transform_matrix": np.asarray(poses[i]).tolist()})
        json.dump({"camera_angle_x": FOV, "frames": frames}, open(os.path.join(root, f"transforms_{subset}.json"), "w"))
    return split["train"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=600)
    ap.add_argument("--steps", type=int, default=300, help="fine-tuning steps per field")
    ap.add_argument("--timed", type=int, default=20, help="further steps timed launch by launch")
    ap.add_argument("--rays", type=int, default=32768, help="rays per fine-tuning step")
    ap.add_argument("--lr-sigma", type=float, default=0.3)
    ap.add_argument("--lr-sh", type=float, default=3e-3)
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps of the baked march")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--resolutions", default="128,256")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd.baked import n_coefficients
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.data.utils import pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene

    degree = 2
    out = {"tool": "baked_finetune_bench", "wh": WH, "steps": args.steps, "rays_per_step": args.rays, "lr_sigma": args.lr_sigma,
           "lr_sh": args.lr_sh, "threshold": args.threshold, "sigma_threshold": args.sigma_threshold, "sh_degree": degree,
           "device": torch.cuda.get_device_name(0)}
    V = N_TRAIN + len(HELD)
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=WH, n_views=V, scale=1.6, compact=True)
    c0.close()
    poses = [pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]          # make_scene's cameras
    root = tempfile.mkdtemp(prefix="knerf_baked_finetune_")
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

    def psnr(imgs):
        v = [float(-10 * np.log10(max(float(((a - b) ** 2).mean()), 1e-20))) for a, b in zip(imgs, truth)]
        return {"min": round(min(v), 2), "mean": round(float(np.mean(v)), 2)}

    mlp = []
    for k in range(0, len(held), 2):                                      # the net is compiled for batches of two images
        i = torch.as_tensor(held[k:k + 2], device="cuda")
        u = torch.rand((2, WH, WH, 128), device="cuda", generator=torch.Generator(device="cuda").manual_seed(100 + k))
        _, fine = nerf.predict_and_render_images((o[i], d[i], t[i]), u=u, outputs=("image",))
        mlp += [x.reshape(-1, 3).clone() for x in fine["image"]]
    out["psnr_held_out"] = {"mlp": psnr(mlp)}

    def baked_views(field):
        return [field.render(a, b, 2.0, 6.0, white_background=True, termination=args.threshold, outputs="image")["image"] for a, b in flat]

    def events(n):
        return [torch.cuda.Event(enable_timing=True) for _ in range(n)]

    W = 1 + 3 * n_coefficients(degree)
    out["fields"] = {}
    for res in (int(r) for r in args.resolutions.split(",") if r):
        field = nerf.bake(resolution=res, sh_degree=degree, sigma_threshold=args.sigma_threshold)
        entry = {"psnr_baked": psnr(baked_views(field)), "step": 0.5 * float(min(field.cell_size))}
        opt = field.optimizer(args.lr_sigma, args.lr_sh, white_background=True, termination=args.threshold)
        entry["slots"], entry["lattice_points"] = opt.n_slots, int(np.prod(field.resolution))
        entry["optimizer_megabytes"] = round(4 * opt.n_slots * W * 4 / 1e6 + 4 * entry["lattice_points"] / 1e6, 1)
        batches = train_ds.ray_batches(args.rays, seed=res)
        torch.cuda.synchronize(); t0 = time.time()
        done, losses = 0, []
        while done < args.steps:                                           # an epoch of the dataset may be shorter than --steps
            hist = opt.fit(batches, 2.0, 6.0, steps=args.steps - done)["loss"]
            if not hist:
                break
            losses += hist; done += len(hist)
        torch.cuda.synchronize()
        entry["fit_seconds"] = round(time.time() - t0, 2)
        entry["loss_first_last"] = [float(np.mean(losses[:10])), float(np.mean(losses[-10:]))]
        entry["psnr_finetuned"] = psnr(baked_views(opt.finish()))
        entry["psnr_live_field"] = psnr(baked_views(opt.field))
        # launch by launch: the gradient launch (with the float64 sum of the per-ray errors behind it) and the Adam launch
        ms_rays, ms_apply, fetched = [], [], []
        for k, (target, (bo, bd, _)) in enumerate(batches):
            if k >= args.timed:
                break
            st = opt.field.render(bo, bd, 2.0, 6.0, white_background=True, termination=args.threshold, outputs="image", stats=True)["stats"]
            e = events(3)
            e[0].record(); opt.accumulate(bo, bd, 2.0, 6.0, target); e[1].record(); opt.apply(); e[2].record()
            e[2].synchronize()
            ms_rays.append(e[0].elapsed_time(e[1])); ms_apply.append(e[1].elapsed_time(e[2])); fetched.append(int(st[0]))
        mr, ma, nf = float(np.median(ms_rays)), float(np.median(ms_apply)), float(np.median(fetched))
        atomic_bytes = nf * 8 * W * 4
        entry["ms_per_step"] = {"gradient_launch": round(mr, 3), "adam_launch": round(ma, 3), "train_step": round(mr + ma, 3)}
        entry["fetched_samples_per_step"] = int(nf)
        entry["atomic_gigabytes_per_second_at_most"] = round(atomic_bytes / (mr * 1e-3) / 1e9, 1)
        entry["adam_gigabytes_per_second"] = round(opt.n_slots * (W * 4 * 7 + 64) / (ma * 1e-3) / 1e9, 1)      # g, m, v, w read and written, a record written
        out["fields"][f"{res}^3"] = entry
        del opt, field
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
