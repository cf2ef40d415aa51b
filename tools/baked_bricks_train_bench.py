"""Fine-tuning a brick baked field as it is against the dense optimiser of the same field, one GPU, one JSON document
(profiles/baked_bricks_train_bench.json with --out).  Scene and protocol of tools/baked_finetune_bench.py: the compact procedural scene
at 128 x 128 (40 training views, 4 held out), the MLP trained for --train-steps steps, baked at degree 2 straight into bricks
(NeRF.bake(bricks=b)), --steps steps of --rays rays.  For every resolution and brick size, S = baked_train.brick_optimizer(bricks) and
D = bricks.to_dense().optimizer(), same rates, fed the same batches:
  - memory, each measured alone and above what is allocated with only the brick field resident, so that the field an optimiser is
    made from counts for neither: the peak over construction (for D the to_dense() table is a temporary of it, released when D
    stands), the bytes allocated once the optimiser stands, the peak over one train_step + finish() from there, and the optimiser's
    own tensors counted (S.nbytes; for D its records, bits, slot tables and rows);
  - rows per slot: stored records / touched records, the share of Adam's rows that are walked and skipped;
  - launch times by HIP events around accumulate() and apply(): S and D alternate step by step (the order swaps every step) over
    --rounds rounds of --steps / --rounds steps each; the median per round, the median of those and their spread (max - min): the
    run-to-run figure a difference has to exceed;
  - PSNR on the held-out views after those steps, both (finish()), and of the field as baked.
Nothing gates on these numbers.

    python tools/baked_bricks_train_bench.py [--train-steps 600] [--steps 300] [--rays 32768] [--out profiles/baked_bricks_train_bench.json]
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
    spec = importlib.util.spec_from_file_location("baked_finetune_bench", os.path.join(ROOT, "tools", "baked_finetune_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=600)
    ap.add_argument("--steps", type=int, default=300, help="fine-tuning steps per optimiser, all of them timed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rays", type=int, default=32768, help="rays per fine-tuning step")
    ap.add_argument("--lr-sigma", type=float, default=0.3)
    ap.add_argument("--lr-sh", type=float, default=3e-3)
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps of the baked march")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--resolutions", default="256,512")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd.baked import BRICKS, n_coefficients, record_bytes
    from keras_nerf_amd.baked_train import brick_optimizer
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.data.utils import pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene
    fb = _finetune_bench()
    WH, N_TRAIN, HELD = fb.WH, fb.N_TRAIN, fb.HELD

    degree = 2
    out = {"tool": "baked_bricks_train_bench", "wh": WH, "steps": args.steps, "rounds": args.rounds, "rays_per_step": args.rays,
           "lr_sigma": args.lr_sigma, "lr_sh": args.lr_sh, "threshold": args.threshold, "sigma_threshold": args.sigma_threshold,
           "sh_degree": degree, "device": torch.cuda.get_device_name(0)}
    V = N_TRAIN + len(HELD)
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=WH, n_views=V, scale=1.6, compact=True)
    c0.close()
    poses = [pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]          # make_scene's cameras
    root = tempfile.mkdtemp(prefix="knerf_baked_bricks_train_")
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

    truth = [img[i].reshape(-1, 3) for i in HELD]
    flat = [(o[i].reshape(-1, 3), d[i].reshape(-1, 3)) for i in HELD]

    def psnr(field):
        imgs = [field.render(a, b, 2.0, 6.0, white_background=True, termination=args.threshold, outputs="image")["image"] for a, b in flat]
        v = [float(-10 * np.log10(max(float(((a - b) ** 2).mean()), 1e-20))) for a, b in zip(imgs, truth)]
        return {"min": round(min(v), 2), "mean": round(float(np.mean(v)), 2)}

    def nbytes(*tensors):
        return sum(int(x.numel()) * x.element_size() for x in tensors)

    def dense_nbytes(opt):
        """what the dense optimiser holds, like BrickFieldOptimizer.nbytes without the field it was made from: its own records and
        bits, the slot tables, flags and four rows"""
        return nbytes(opt.field._records, opt.field._words, opt._slot_of, opt._point_of, opt._index, opt._trainable,
                      opt._master, opt._grad, opt._m, opt._v)

    kw = dict(white_background=True, termination=args.threshold)

    def build(kind, bricks):
        if kind == "brick":
            return brick_optimizer(bricks, args.lr_sigma, args.lr_sh, **kw), None
        dense = bricks.to_dense()
        return dense.optimizer(args.lr_sigma, args.lr_sh, **kw), dense

    def peak(kind, bricks, batch):
        """Memory of one optimiser alone, all above what is allocated with only the brick field resident (the field an optimiser is
        made from is counted for neither): the peak over construction (for the dense one the to_dense() table is a temporary of the
        construction and is released with it), the bytes allocated once it stands, the peak over one train_step + finish() from
        there, and the optimiser's own tensors counted"""
        target, (bo, bd, _) = batch
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        opt, dense = build(kind, bricks)
        del dense
        torch.cuda.synchronize()
        res = {"construction_peak_bytes": int(torch.cuda.max_memory_allocated() - base),
               "allocated_after_construction_bytes": int(torch.cuda.memory_allocated() - base)}
        torch.cuda.reset_peak_memory_stats()
        opt.train_step(bo, bd, 2.0, 6.0, target)
        done = opt.finish()
        torch.cuda.synchronize()
        res["step_and_finish_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        res["optimizer_bytes"] = int(opt.nbytes if kind == "brick" else dense_nbytes(opt))
        del opt, done
        return res

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record(); b.synchronize()
        return a.elapsed_time(b)

    out["fields"] = {}
    per_round = max(1, args.steps // args.rounds)
    for res in (int(r) for r in args.resolutions.split(",") if r):
        for b in BRICKS:
            bricks = nerf.bake(resolution=res, sh_degree=degree, sigma_threshold=args.sigma_threshold, bricks=b)
            entry = {"psnr_baked": psnr(bricks), "step": 0.5 * float(min(bricks.cell_size)), "brick_field_bytes": bricks.nbytes,
                     "n_bricks": bricks.n_bricks, "dense_table_bytes": res ** 3 * record_bytes(degree)}
            batches = iter(train_ds.ray_batches(args.rays, seed=res))

            def batch():
                nonlocal batches
                try:
                    return next(batches)
                except StopIteration:                                       # an epoch of the dataset may be shorter than the run
                    batches = iter(train_ds.ray_batches(args.rays, seed=res + 1))
                    return next(batches)
            first = batch()
            entry["memory"] = {kind: peak(kind, bricks, first) for kind in ("brick", "dense")}
            opts = {}
            opts["brick"], _ = build("brick", bricks)
            opts["dense"], dense = build("dense", bricks)
            S = opts["brick"]
            stored = S.field.n_bricks * b ** 3
            entry.update(slots=S.n_slots, stored_records=stored, rows_per_slot=round(stored / S.n_slots, 4), dense_slots=opts["dense"].n_slots)
            for kind in opts:                                              # warm-up: one step each, not timed
                target, (bo, bd, _) = first
                opts[kind].train_step(bo, bd, 2.0, 6.0, target)
            medians = {k: {"gradient": [], "adam": []} for k in opts}
            step = 0
            for _ in range(args.rounds):
                ms = {k: {"gradient": [], "adam": []} for k in opts}
                for _ in range(per_round):
                    target, (bo, bd, _) = batch()
                    for kind in (("brick", "dense") if step % 2 == 0 else ("dense", "brick")):
                        opt = opts[kind]
                        ms[kind]["gradient"].append(timed(lambda: opt.accumulate(bo, bd, 2.0, 6.0, target)))
                        ms[kind]["adam"].append(timed(opt.apply))
                    step += 1
                for kind in opts:
                    for what in ("gradient", "adam"):
                        medians[kind][what].append(float(np.median(ms[kind][what])))
            entry["timed_steps"] = step
            entry["ms"] = {}
            for kind in opts:
                entry["ms"][kind] = {}
                for what in ("gradient", "adam"):
                    m = medians[kind][what]
                    entry["ms"][kind][what + "_launch"] = {"ms": round(float(np.median(m)), 4), "round_medians_ms": [round(v, 4) for v in m],
                                                           "spread_ms": round(max(m) - min(m), 4)}
            entry["psnr_finetuned"] = {kind: psnr(opts[kind].finish()) for kind in opts}
            print(f"{res}^3 b={b}: {json.dumps(entry)}", file=sys.stderr, flush=True)
            out["fields"][f"{res}^3 b={b}"] = entry
            del opts, S, dense, bricks, opt
            torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
