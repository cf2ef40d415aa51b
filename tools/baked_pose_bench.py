"""Refining camera poses against a baked field, one GPU, one JSON document (profiles/baked_pose_bench.json with --out), on the scene of
tools/baked_finetune_bench.py (the compact procedural scene at 128 x 128, 40 training views and 4 held out, the MLP trained as there,
baked at --resolution^3, degree 2):
  (a) milliseconds of the ray-gradient launch (knerf_baked_ray_gradients, dense and through bricks of 8) and of the reduction to
      cameras (knerf_pose_gradients) beside the optimiser's gradient launch (knerf_baked_train_rays / knerf_baked_bricks_train_rays)
      on the same --rays rays of the dataset: device events around each launch, --warmup launches first, the median and the spread
      (min, max) over --reps, the launches taken in turns so that a drift of the machine hits all of them alike;
  (b) pose recovery: the training cameras turned by --degrees about random axes and moved by --shift (scene units), then --steps steps
      of (1) fine-tuning the field alone on rays drawn with the perturbed cameras and (2) field and cameras together
      (baked_pose.fit_with_poses), per seed: PSNR on the held-out views rendered at their TRUE poses, and the mean rotation and
      translation error of the training cameras before and after.  No camera is fixed: the baked field itself ties the frame down.
Nothing gates on these numbers; they are reported as they come out.

    python tools/baked_pose_bench.py [--train-steps 600] [--steps 300] [--rays 32768] [--out profiles/baked_pose_bench.json]
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _finetune_bench():
    """tools/baked_finetune_bench.py as a module: the scene's layout on disk is written by its write_scene"""
    spec = importlib.util.spec_from_file_location("baked_finetune_bench", os.path.join(ROOT, "tools", "baked_finetune_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=600)
    ap.add_argument("--steps", type=int, default=300, help="fine-tuning steps per run of (b)")
    ap.add_argument("--rays", type=int, default=32768)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--seeds", default="0,1,2")
    ap.add_argument("--degrees", type=float, default=1.0)
    ap.add_argument("--shift", type=float, default=0.04)
    ap.add_argument("--lr-sigma", type=float, default=0.3)
    ap.add_argument("--lr-sh", type=float, default=3e-3)
    ap.add_argument("--lr-rotation", type=float, default=5e-4)
    ap.add_argument("--lr-translation", type=float, default=1e-3)
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps of the baked march")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd import baked_pose, baked_train
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.data.utils import pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.baked_pose_reference import move_poses
    from tests.procedural_scene import make_scene

    fb = _finetune_bench()
    WH, N_TRAIN, HELD = fb.WH, fb.N_TRAIN, fb.HELD
    degree = 2
    out = {"tool": "baked_pose_bench", "wh": WH, "resolution": args.resolution, "sh_degree": degree, "rays": args.rays,
           "threshold": args.threshold, "sigma_threshold": args.sigma_threshold, "device": torch.cuda.get_device_name(0)}
    V = N_TRAIN + len(HELD)
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=WH, n_views=V, scale=1.6, compact=True)
    c0.close()
    poses = [pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]          # make_scene's cameras
    root = tempfile.mkdtemp(prefix="knerf_baked_pose_")
    train_views = torch.as_tensor(fb.write_scene(root, img.cpu().numpy(), poses), device="cuda")
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
    field = nerf.bake(resolution=args.resolution, sh_degree=degree, sigma_threshold=args.sigma_threshold)
    bricks = field.compact(8)
    march = dict(white_background=True, termination=args.threshold)

    held = list(HELD)
    truth = [img[i].reshape(-1, 3) for i in held]
    flat = [(o[i].reshape(-1, 3), d[i].reshape(-1, 3)) for i in held]

    def psnr(f):
        v = [float(-10 * np.log10(max(float(((f.render(a, b, 2.0, 6.0, outputs="image", **march)["image"] - c) ** 2).mean()), 1e-20)))
             for (a, b), c in zip(flat, truth)]
        return {"min": round(min(v), 2), "mean": round(float(np.mean(v)), 2)}

    # ---- (a) the launches side by side on one batch of the dataset
    batches = train_ds.ray_batches(args.rays, seed=1)
    batches.set_cameras(lambda: batches._resident_all()[1])                # the stored cameras; the hook is on for last_view
    target, (bo, bd, _) = next(iter(batches))
    view = batches.last_view
    n_views = int(batches.n_views)
    opt_d = field.optimizer(args.lr_sigma, args.lr_sh, **march)
    opt_b = baked_train.brick_optimizer(bricks, args.lr_sigma, args.lr_sh, **march)
    go, gd, _ = opt_d.field.ray_gradients(bo, bd, 2.0, 6.0, target, **march)
    launches = {
        "train_rays_dense": lambda: opt_d.accumulate(bo, bd, 2.0, 6.0, target),
        "ray_gradients_dense": lambda: opt_d.field.ray_gradients(bo, bd, 2.0, 6.0, target, **march),
        "train_rays_bricks": lambda: opt_b.accumulate(bo, bd, 2.0, 6.0, target),
        "ray_gradients_bricks": lambda: opt_b.field.ray_gradients(bo, bd, 2.0, 6.0, target, **march),
        "pose_gradients": lambda: baked_pose.pose_gradients(go, gd, bd, view, n_views),
    }
    ms = {k: [] for k in launches}
    for rep in range(args.warmup + args.reps):
        for name, fn in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    timing = {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}
    for kind in ("dense", "bricks"):
        timing[f"ratio_ray_gradients_over_train_rays_{kind}"] = round(
            timing[f"ray_gradients_{kind}"]["median_ms"] / timing[f"train_rays_{kind}"]["median_ms"], 3)
    st = field.render(bo, bd, 2.0, 6.0, outputs="image", stats=True, **march)["stats"]
    timing["fetched_samples"] = int(st[0])
    timing["note"] = ("each figure is one launch with the float64 sum of the per-ray errors behind it (pose_gradients: the launch alone); "
                      f"{args.warmup} warm-up and {args.reps} timed repetitions, the five launches in turns")
    out["launches"] = timing
    del opt_d, opt_b

    # ---- (b) perturbed training cameras: the field alone against field and cameras
    true_cams = batches._resident_all()[1].clone()
    out["psnr_held_out_baked"] = psnr(field)
    runs = []

    def fit(run_fit, steps):
        done, losses = 0, []
        while done < steps:                                                # an epoch of the dataset may be shorter than --steps
            hist = run_fit(steps - done)
            if not hist:
                break
            losses += hist; done += len(hist)
        return losses

    for seed in (int(s) for s in args.seeds.split(",") if s != ""):
        rng = np.random.default_rng(seed)
        axis = rng.standard_normal((N_TRAIN, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        move = rng.standard_normal((N_TRAIN, 3)); move /= np.linalg.norm(move, axis=1, keepdims=True)
        start = torch.as_tensor(move_poses(true_cams.cpu().numpy(), np.radians(args.degrees) * axis, args.shift * move).astype(np.float32)).cuda()
        r0, t0_ = (float(e.mean()) for e in baked_pose.pose_errors(start, true_cams))
        entry = {"seed": seed, "rotation_error_degrees_start": round(r0, 4), "translation_error_start": round(t0_, 5)}
        # (1) the field alone, its rays drawn with the perturbed cameras
        ds = train_ds.ray_batches(args.rays, seed=100 + seed)
        ds.set_cameras(lambda: start)
        opt = field.optimizer(args.lr_sigma, args.lr_sh, **march)
        torch.cuda.synchronize(); t1 = time.time()
        losses = fit(lambda n: opt.fit(ds, 2.0, 6.0, steps=n)["loss"], args.steps)
        torch.cuda.synchronize()
        entry["field_only"] = {"psnr_held_out": psnr(opt.finish()), "seconds": round(time.time() - t1, 2),
                               "loss_first_last": [float(np.mean(losses[:10])), float(np.mean(losses[-10:]))]}
        # (2) field and cameras
        ds = train_ds.ray_batches(args.rays, seed=100 + seed)
        opt = field.optimizer(args.lr_sigma, args.lr_sh, **march)
        po = baked_pose.PoseOptimizer(start, args.lr_rotation, args.lr_translation)
        torch.cuda.synchronize(); t1 = time.time()
        losses = fit(lambda n: baked_pose.fit_with_poses(opt, po, ds, 2.0, 6.0, steps=n)["loss"], args.steps)
        torch.cuda.synchronize()
        r1, t1_ = (float(e.mean()) for e in baked_pose.pose_errors(po.poses, true_cams))
        entry["joint"] = {"psnr_held_out": psnr(opt.finish()), "seconds": round(time.time() - t1, 2),
                          "loss_first_last": [float(np.mean(losses[:10])), float(np.mean(losses[-10:]))],
                          "rotation_error_degrees_end": round(r1, 4), "translation_error_end": round(t1_, 5)}
        runs.append(entry)
        del opt, po
    out["pose_recovery"] = {"degrees": args.degrees, "shift": args.shift, "steps": args.steps, "lr_sigma": args.lr_sigma, "lr_sh": args.lr_sh,
                            "lr_rotation": args.lr_rotation, "lr_translation": args.lr_translation, "runs": runs}
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
