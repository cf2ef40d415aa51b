"""The baked field against the MLP renderer, one GPU, one JSON document (profiles/baked_bench.json with --out):
  - NeRF.bake at 128^3 and 256^3, degree 2: seconds (device-synchronised wall clock), occupied cells, lattice points fitted;
  - 256 x 256 views on poses pose_spherical(theta, -30, 4): median frame time of BakedField.render (termination --threshold, empty
    cells skipped) for every kernel variant of the degree (lanes per ray: include/knerf.h), with skipping off, and the fraction of
    samples fetched, against NeRF.predict_and_render_images with build_occupancy_grid(--grid) and set_ray_termination(--threshold);
  - PSNR of the baked views against the MLP's fine image (dense render, no grid, no termination) for degree 0, 1 and 2.

    python tools/baked_bench.py [--train-steps 600] [--frames 12] [--out profiles/baked_bench.json] [--model_dirs coarse.h5,fine.h5]

Without --model_dirs it trains the compact procedural scene (tests/procedural_scene.py) at 128 x 128 for --train-steps steps, as
tools/termination_bench.py does.
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
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps of both renderers")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--grid", type=int, default=128, help="cells per axis of the MLP renderer's occupancy grid")
    ap.add_argument("--resolutions", default="128,256")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--model_dirs", default="", help="coarse.h5,fine.h5")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd.baked import LANES
    from keras_nerf_amd.data.utils import get_focal_from_fov, pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import FOV, make_scene

    wh = 256
    out = {"tool": "baked_bench", "wh": wh, "frames": args.frames, "threshold": args.threshold, "sigma_threshold": args.sigma_threshold,
           "grid": args.grid, "device": torch.cuda.get_device_name(0)}
    nerf = NeRF(seed=0)
    if args.model_dirs:
        c, f = args.model_dirs.split(",")
        nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=1, image_height=wh, image_width=wh, ray_chunks=4096, white_background=True)
        nerf.coarse.load_weights(c); nerf.fine.load_weights(f)
        out["weights"] = "model_dirs"
    else:
        tw, batch = 128, 2
        c0 = KnerfContext(white_background=True)
        o, d, t, img = make_scene(c0, wh=tw, n_views=40, scale=1.6, compact=True)
        c0.close()
        trainer = NeRF(seed=0)
        trainer.compile({"learning_rate": 5e-4}, "mse", batch_size=batch, image_height=tw, image_width=tw, ray_chunks=4096,
                        white_background=True)
        order = np.random.default_rng(5).integers(0, 40, (args.train_steps, batch))
        t0 = time.time()
        for s in range(args.train_steps):
            idx = torch.as_tensor(order[s], device="cuda")
            trainer.train_step((img[idx], (o[idx], d[idx], t[idx])), with_metrics=False)
        trainer._ctx.poll_nonfinite(wait=True)
        out["train"] = f"compact procedural scene, {tw}x{tw}, batch {batch}, {args.train_steps} steps ({time.time() - t0:.1f} s)"
        del o, d, t, img
        nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=1, image_height=wh, image_width=wh, ray_chunks=4096, white_background=True)
        nerf.coarse.set_flat_weights(trainer.coarse.get_flat_weights()); nerf.fine.set_flat_weights(trainer.fine.get_flat_weights())
        trainer._ctx.close()

    focal = get_focal_from_fov(FOV, wh)
    rays = []
    for i in range(args.frames):
        c2w = pose_spherical(360.0 * i / args.frames, -30.0, 4.0)
        o, d, t = nerf._ctx.generate_rays(np.asarray(c2w, np.float32), focal, wh, wh, 2.0, 6.0, 64, None, seed=i)
        u = torch.rand((1, wh, wh, 128), device="cuda", generator=torch.Generator(device="cuda").manual_seed(100 + i))
        rays.append(((o, d, t), u))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record(); b.synchronize()
        return a.elapsed_time(b), r

    def mlp_sweep():
        nerf.predict_and_render_images(rays[0][0], u=rays[0][1], outputs=("image", "depth"))          # warm-up (workspaces)
        ms, imgs = [], []
        for r, u in rays:
            dt, (_, fine) = timed(lambda: nerf.predict_and_render_images(r, u=u, outputs=("image", "depth")))
            ms.append(dt); imgs.append(fine["image"].reshape(-1, 3).clone())
        return float(np.median(ms)), imgs

    def psnr(imgs, ref):
        v = [float(-10 * np.log10(max(float(((a - b) ** 2).mean()), 1e-20))) for a, b in zip(imgs, ref)]
        return {"min": round(min(v), 2), "mean": round(float(np.mean(v)), 2)}

    _, dense = mlp_sweep()
    nerf.build_occupancy_grid(args.grid)
    nerf.set_ray_termination(args.threshold)
    mlp_ms, mlp_imgs = mlp_sweep()
    nerf.set_ray_termination(0); nerf.clear_occupancy_grid()
    out["mlp_grid_termination"] = {"ms": round(mlp_ms, 3), "fps": round(1e3 / mlp_ms, 1), "psnr_vs_dense": psnr(mlp_imgs, dense)}

    def baked_sweep(field, **kw):
        flat = [(r[0].reshape(-1, 3), r[1].reshape(-1, 3)) for r, _ in rays]
        field.render(*flat[0], 2.0, 6.0, white_background=True, termination=args.threshold, **kw)      # warm-up
        ms, imgs, fetched, total = [], [], 0, 0
        for o, d in flat:
            dt, res = timed(lambda: field.render(o, d, 2.0, 6.0, white_background=True, termination=args.threshold, stats=True,
                                                 outputs=("image", "depth"), **kw))
            ms.append(dt); imgs.append(res["image"])
            st = res["stats"].cpu().numpy()
            fetched += int(st[0]); total += int(st[1])
        return float(np.median(ms)), imgs, fetched / max(total, 1)

    out["bake"], out["render"] = {}, {}
    for res in (int(r) for r in args.resolutions.split(",") if r):
        for degree in ((2, 1, 0) if res == 256 else (2,)):
            torch.cuda.synchronize(); t0 = time.time()
            field = nerf.bake(resolution=res, sh_degree=degree, sigma_threshold=args.sigma_threshold)
            torch.cuda.synchronize(); sec = time.time() - t0
            key = f"{res}^3 degree {degree}"
            occ = field.occupied
            out["bake"][key] = {"seconds": round(sec, 3), "occupied_cells": round(float(occ.float().mean()), 4),
                                "record_megabytes": round(field._records.numel() / 1e6, 1), "step": 0.5 * float(min(field.cell_size))}
            entry = {}
            for lanes in LANES[degree]:
                ms, imgs, frac = baked_sweep(field, lanes_per_ray=lanes)
                entry[f"lanes_{lanes}"] = {"ms": round(ms, 3), "fps": round(1e3 / ms, 1), "vs_mlp": round(mlp_ms / ms, 2),
                                           "fetched": round(frac, 4), "psnr_vs_mlp_dense": psnr(imgs, dense)}
            ms, imgs, frac = baked_sweep(field, skip_empty=False)
            entry["default_no_skip"] = {"ms": round(ms, 3), "fetched": round(frac, 4)}
            ms0, imgs0, _ = baked_sweep(field)
            entry["default"] = {"ms": round(ms0, 3), "skip_bit_identical": all(bool(torch.equal(a, b)) for a, b in zip(imgs, imgs0))}
            out["render"][key] = entry
            del field
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
