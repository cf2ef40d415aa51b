"""Depth supervision of the grid optimisers, one GPU, one JSON document (profiles/baked_depth_bench.json with --out).  Scene and protocol
are those of tools/baked_coarse_to_fine_bench.py: the compact procedural scene at 128 x 128, 40 training views and 4 held out, the MLP
trained --train-steps steps, degree 2, termination 1e-4, white background.  Nothing gates on these numbers.

Launch cost: the gradient launch of one batch of --rays rays on the bake at 128^3 and at 256^3, dense and as bricks (compact(8)), through
  rgba           knerf_baked[_bricks]_train_rays_rgba (a background per ray), this build
  depth          knerf_baked[_bricks]_train_rays_depth (the same, and a depth target and weight per ray), this build
  parent_rgba    the rgba launch of the library given with --parent-lib (a build of the parent commit), when there is one
alternated launch by launch in one process, --timed rounds after two warm-up rounds; milliseconds by device events around accumulate():
median, 10th and 90th percentile.

Effect: the BakedField.uniform route (stages 64^3 -> 127^3 -> 253^3, TV on, --steps steps in all; run (d) of the coarse-to-fine tool)
without depth and with depth_loss in --depth-loss, for --seeds batch seeds.  The teacher is the bake at 256^3 after --steps steps of
fine-tuning; its depth, rendered along the dataset's own rays, is the target: dense (every pixel, weight 1) and sparse (1 % of the
pixels have weight 1, the others 0).  Per run: held-out PSNR against ground truth and the RMSE of the depth against the teacher's on the
held-out views.

    python tools/baked_depth_bench.py [--parent-lib PATH] [--out profiles/baked_depth_bench.json]
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


class Batches:
    """ray batches without end, one epoch of the dataset after the other, with the current epoch's last_depth readable"""

    def __init__(self, dataset, rays, seed, depth=None, weight=None):
        self._args, self._seed, self._now = (dataset, rays, depth, weight), seed, None

    @property
    def last_depth(self):
        return None if self._now is None else self._now.last_depth

    def __iter__(self):
        dataset, rays, depth, weight = self._args
        while True:
            self._now = dataset.ray_batches(rays, seed=self._seed, depth=depth, depth_weight=weight)
            n = 0
            for b in self._now:
                n += 1
                yield b
            if not n:
                return
            self._seed += 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=600)
    ap.add_argument("--steps", type=int, default=300, help="ray-batch steps of every run, all stages together")
    ap.add_argument("--timed", type=int, default=30, help="timed rounds of the launch-cost part")
    ap.add_argument("--rays", type=int, default=32768, help="rays per step")
    ap.add_argument("--lr-sigma", type=float, default=0.3)
    ap.add_argument("--lr-sh", type=float, default=3e-3)
    ap.add_argument("--tv-sigma", type=float, default=1e-5)
    ap.add_argument("--tv-sh", type=float, default=1e-3)
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps of the baked march")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--depth-loss", default="0.01,0.1,1.0")
    ap.add_argument("--seeds", default="7,8,9")
    ap.add_argument("--sparse-fraction", type=float, default=0.01)
    ap.add_argument("--parent-lib", default="", help="libknerf_hip.so of the parent commit, for the third column of the launch cost")
    ap.add_argument("--parts", default="launch,effect")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from baked_finetune_bench import HELD, N_TRAIN, WH, write_scene
    from keras_nerf_amd import _lib
    from keras_nerf_amd.baked import BakedField
    from keras_nerf_amd.baked_train import brick_optimizer, fit_coarse_to_fine
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.data.utils import pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene

    degree = 2
    bounds = ((-1.5,) * 3, (1.5,) * 3)
    tv = dict(tv_sigma=args.tv_sigma, tv_sh=args.tv_sh, tv_epsilon=1e-6)
    march = dict(white_background=True, termination=args.threshold)
    out = {"tool": "baked_depth_bench", "wh": WH, "steps": args.steps, "rays_per_step": args.rays, "lr_sigma": args.lr_sigma,
           "lr_sh": args.lr_sh, "tv": tv, "threshold": args.threshold, "sigma_threshold": args.sigma_threshold, "sh_degree": degree,
           "device": torch.cuda.get_device_name(0)}
    V = N_TRAIN + len(HELD)
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=WH, n_views=V, scale=1.6, compact=True)
    c0.close()
    poses = [pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]
    root = tempfile.mkdtemp(prefix="knerf_baked_depth_")
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
    kw = dict(learning_rate_sigma=args.lr_sigma, learning_rate_sh=args.lr_sh, **march)

    # the teacher: the bake at 256^3, fine-tuned on the photographs
    f256 = nerf.bake(resolution=256, sh_degree=degree, sigma_threshold=args.sigma_threshold)
    teacher, _ = fit_coarse_to_fine(f256, Batches(train_ds, args.rays, 7), 2.0, 6.0, [(None, args.steps)], **kw)
    render = lambda field, a, b, what: field.render(a, b, 2.0, 6.0, outputs=what, **march)[what]
    teacher_held = [render(teacher, a, b, "depth") for a, b in flat]

    def score(field):
        v = [float(-10 * np.log10(max(float(((render(field, a, b, "image") - g) ** 2).mean()), 1e-20))) for (a, b), g in zip(flat, truth)]
        z = [float(((render(field, a, b, "depth") - g) ** 2).mean()) for (a, b), g in zip(flat, teacher_held)]
        return {"psnr_min": round(min(v), 2), "psnr_mean": round(float(np.mean(v)), 2), "depth_rmse": round(float(np.sqrt(np.mean(z))), 4)}

    out["teacher"] = {"what": f"bake at 256^3, {args.steps} steps of fine-tuning", **score(teacher)}
    # its depth along the dataset's own rays, view by view: the unit of the optimisers' depth targets
    rg = train_ds._rg_factory(0)
    maps = []
    for pose in train_ds.camera_params:
        ov, dv, _ = rg(pose)
        maps.append(render(teacher, ov.reshape(-1, 3), dv.reshape(-1, 3), "depth").reshape(WH, WH))
    depth_map = torch.stack(maps)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    sparse_weight = (torch.rand(depth_map.shape, device="cuda", generator=gen) < args.sparse_fraction).to(torch.float32)
    out["depth_maps"] = {"views": len(maps), "mean_teacher_depth": round(float(depth_map.mean()), 4),
                         "sparse_pixels": int(sparse_weight.sum()), "pixels": int(sparse_weight.numel())}

    if "launch" in args.parts:
        parent = None
        if args.parent_lib:                                 # (the parent has no _depth entry points: only its rgba launches are bound)
            import ctypes
            parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
            for name in ("knerf_baked_train_rays_rgba", "knerf_baked_bricks_train_rays_rgba"):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        ours = _lib.load()
        target, (bo, bd, _) = next(iter(train_ds.ray_batches(args.rays, seed=3)))
        n = bo.shape[0]
        bg = torch.rand((n, 3), device="cuda", generator=gen)
        z = render(teacher, bo, bd, "depth")
        c = torch.ones_like(z)
        out["launch_ms"] = {"rays": n, "timed_rounds": args.timed, "parent_lib": bool(parent),
                            "what": "median [p10, p90] of accumulate() by device events, versions alternated launch by launch"}
        for res in (128, 256):
            base = f256 if res == 256 else nerf.bake(resolution=128, sh_degree=degree, sigma_threshold=args.sigma_threshold)
            for storage in ("dense", "bricks"):
                make = (lambda **k: base.optimizer(args.lr_sigma, args.lr_sh, **march, **k)) if storage == "dense" else \
                    (lambda **k: brick_optimizer(base.compact(8), args.lr_sigma, args.lr_sh, **march, **k))
                opts = {"rgba": make(), "depth": make(depth_loss=0.1)}
                if parent is not None:
                    opts["parent_rgba"] = make()
                ms = {k: [] for k in opts}
                for r in range(args.timed + 2):
                    for name, opt in opts.items():
                        extra = dict(depth=z, depth_weight=c) if name == "depth" else {}
                        _lib_load = _lib.load
                        if name == "parent_rgba":
                            _lib.load = lambda: parent
                        try:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(); opt.accumulate(bo, bd, 2.0, 6.0, target, background=bg, **extra); e1.record(); e1.synchronize()
                        finally:
                            _lib.load = _lib_load
                        if r >= 2:
                            ms[name].append(e0.elapsed_time(e1))
                        opt._grad.zero_()
                assert tuple(opts["depth"].objective_terms())[-1] == "depth" and tuple(opts["rgba"].objective_terms())[-1] == "opacity"
                out["launch_ms"][f"{storage}_{res}"] = {
                    "slots": opts["rgba"].n_slots,
                    **{k: [round(float(np.median(v)), 3), round(float(np.percentile(v, 10)), 3), round(float(np.percentile(v, 90)), 3)]
                       for k, v in ms.items()}}
                del opts
            del base
        assert ours is _lib.load()
    del f256

    if "effect" in args.parts:
        third = args.steps // 3
        stages = [(None, third), (127, third), (253, args.steps - 2 * third)]
        lambdas = [float(x) for x in args.depth_loss.split(",") if x]
        out["effect"] = {"route": "BakedField.uniform(64, sigma 0.1, colour 0.5), stages 64^3 -> 127^3 -> 253^3, TV on", "runs": []}
        for seed in (int(x) for x in args.seeds.split(",") if x):
            variants = [("none", 0.0, None, None)] + [("dense", lam, depth_map, None) for lam in lambdas] + \
                       [("sparse", lam, depth_map, sparse_weight) for lam in lambdas]
            for name, lam, zmap, wmap in variants:
                start = BakedField.uniform(64, bounds, degree, sigma=0.1, colour=0.5)
                torch.cuda.synchronize(); t0 = time.time()
                field, hist = fit_coarse_to_fine(start, Batches(train_ds, args.rays, seed, zmap, wmap), 2.0, 6.0, stages, **kw, **tv,
                                                 **({"depth_loss": lam} if lam else {}))
                torch.cuda.synchronize()
                entry = {"seed": seed, "depth": name, "depth_loss": lam, "fit_seconds": round(time.time() - t0, 2),
                         "loss_first_last": [float(np.mean(hist["loss"][:10])), float(np.mean(hist["loss"][-10:]))], **score(field)}
                if lam:
                    entry["depth_term_first_last"] = [float(np.mean(hist["depth"][:10])), float(np.mean(hist["depth"][-10:]))]
                out["effect"]["runs"].append(entry)
                print(json.dumps(entry), flush=True)
        # the table: mean and spread over the seeds per variant
        table = {}
        for e in out["effect"]["runs"]:
            table.setdefault(f"{e['depth']} {e['depth_loss']}", []).append(e)
        out["effect"]["table"] = {k: {"psnr_mean": [round(float(np.mean([e["psnr_mean"] for e in v])), 2), min(e["psnr_mean"] for e in v),
                                                    max(e["psnr_mean"] for e in v)],
                                      "depth_rmse": [round(float(np.mean([e["depth_rmse"] for e in v])), 4), min(e["depth_rmse"] for e in v),
                                                     max(e["depth_rmse"] for e in v)]} for k, v in table.items()}
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
