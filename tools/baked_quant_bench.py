"""The brick baked field with 8-bit SH coefficients against the brick field it was quantised from, one GPU, one JSON document
(profiles/baked_quant_bench.json with --out).  Protocol of tools/baked_bricks_bench.py: the compact procedural scene (40 training views
and 4 held out, 128 x 128) trained for --train-steps steps, baked at degree 2 straight into bricks of 8^3 at 256^3 and 512^3, 256 x 256
views on poses pose_spherical(theta, -30, 4), white background, termination --threshold, step = half a cell.  For the BrickBakedField
and its QuantizedBrickField:
  - bytes on the device (records + exponents + brick table + bits) and in the saved file;
  - quantize() and dequantize() seconds (device-synchronised wall clock, the median of five after a warm-up call);
  - frame time: HIP events around render(), --frames poses per round, the brick kernel (the untouched launch of csrc/baked.hip at
    its default variant) and every variant of the quantised kernel alternating in rotating order inside every pose, after a warm-up
    render of each; the median per round, --rounds rounds, and the spread of the rounds' medians (max - min): the run-to-run figure a
    difference between two of them has to exceed;
  - PSNR of the quantised views against the brick field's views on those poses, and of both against the held-out ground truth;
  - whether lanes_per_ray=1 on the quantised field gives the bits of lanes_per_ray=1 on dequantize(), and whether
    dequantize().quantize() gives the quantised bytes back.

    python tools/baked_quant_bench.py [--train-steps 600] [--frames 20] [--rounds 5] [--out profiles/baked_quant_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=600)
    ap.add_argument("--threshold", type=float, default=1e-4, help="termination eps")
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--brick", type=int, default=8)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd.baked_quant import QLANES
    from keras_nerf_amd.data.utils import get_focal_from_fov, pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import FOV, make_scene

    wh, tw, batch, n_train, n_held = 256, 128, 2, 40, 4
    out = {"tool": "baked_quant_bench", "wh": wh, "frames": args.frames, "rounds": args.rounds, "threshold": args.threshold,
           "sigma_threshold": args.sigma_threshold, "degree": args.degree, "brick": args.brick, "device": torch.cuda.get_device_name(0)}
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=tw, n_views=n_train + n_held, scale=1.6, compact=True)
    c0.close()
    trainer = NeRF(seed=0)
    trainer.compile({"learning_rate": 5e-4}, "mse", batch_size=batch, image_height=tw, image_width=tw, ray_chunks=4096, white_background=True)
    order = np.random.default_rng(5).integers(0, n_train, (args.train_steps, batch))
    t0 = time.time()
    for s in range(args.train_steps):
        idx = torch.as_tensor(order[s], device="cuda")
        trainer.train_step((img[idx], (o[idx], d[idx], t[idx])), with_metrics=False)
    trainer._ctx.poll_nonfinite(wait=True)
    out["train"] = (f"compact procedural scene, {tw}x{tw}, batch {batch}, {args.train_steps} steps on {n_train} views, {n_held} held out "
                    f"({time.time() - t0:.1f} s)")
    held = [(o[i].reshape(-1, 3).contiguous(), d[i].reshape(-1, 3).contiguous(), img[i].reshape(-1, 3)) for i in range(n_train, n_train + n_held)]
    del o, d, t, img
    nerf = NeRF(seed=0)
    nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=1, image_height=wh, image_width=wh, ray_chunks=4096, white_background=True)
    nerf.coarse.set_flat_weights(trainer.coarse.get_flat_weights()); nerf.fine.set_flat_weights(trainer.fine.get_flat_weights())
    trainer._ctx.close()

    focal = get_focal_from_fov(FOV, wh)
    rays = []
    for i in range(args.frames):
        c2w = pose_spherical(360.0 * i / args.frames, -30.0, 4.0)
        ro, rd, _ = nerf._ctx.generate_rays(np.asarray(c2w, np.float32), focal, wh, wh, 2.0, 6.0, 64, None, seed=i)
        rays.append((ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()))

    def wall(fn, repeat=5):
        fn()                                                                               # warm-up: allocator
        secs = []
        for _ in range(repeat):
            torch.cuda.synchronize(); t0 = time.time()
            r = fn()
            torch.cuda.synchronize()
            secs.append(time.time() - t0)
            del r
        return float(np.median(secs))

    def render(field, ro, rd, outputs=("image", "depth"), **kw):
        return field.render(ro, rd, 2.0, 6.0, white_background=True, termination=args.threshold, outputs=outputs, **kw)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record(); b.synchronize()
        return a.elapsed_time(b)

    def file_bytes(field):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "field.npz")
            field.save(path)
            return os.path.getsize(path)

    def psnr(a, b):
        return float(-10.0 * np.log10(max(float(((a.double() - b.double()) ** 2).mean()), 1e-20)))

    def sweep(variants):
        """frame times per (field, lanes_per_ray): rounds x frames, the variants alternating in rotating order inside every pose"""
        names = list(variants)
        for n in names:
            f, lanes = variants[n]
            render(f, *rays[0], lanes_per_ray=lanes); render(f, *rays[0], lanes_per_ray=lanes)         # warm-up
        medians = {n: [] for n in names}
        for _ in range(args.rounds):
            ms = {n: [] for n in names}
            for i, (ro, rd) in enumerate(rays):
                for j in range(len(names)):
                    n = names[(i + j) % len(names)]
                    f, lanes = variants[n]
                    ms[n].append(timed(lambda: render(f, ro, rd, lanes_per_ray=lanes)))
            for n in names:
                medians[n].append(float(np.median(ms[n])))
        res = {}
        for n in names:
            m = medians[n]
            res[n] = {"ms": round(float(np.median(m)), 4), "round_medians_ms": [round(v, 4) for v in m],
                      "spread_ms": round(max(m) - min(m), 4)}
        return res

    def measure(res):
        kw = dict(resolution=res, sh_degree=args.degree, sigma_threshold=args.sigma_threshold, bricks=args.brick)
        bricks = nerf.bake(**kw)
        q = bricks.quantize()
        entry = {"n_bricks": bricks.n_bricks, "stored_records": bricks.n_bricks * bricks.brick ** 3,
                 "step": 0.5 * float(min(bricks.cell_size))}
        entry["device_bytes"] = {"bricks": bricks.nbytes, "quantised": q.nbytes,
                                 "bricks_records": int(bricks._records.numel()), "quantised_records": int(q._records.numel()),
                                 "exponents": 4 * int(q.exponents.numel())}
        entry["device_bytes"]["quantised_over_bricks"] = round(q.nbytes / bricks.nbytes, 4)
        entry["file_bytes"] = {"bricks": file_bytes(bricks), "quantised": file_bytes(q)}
        entry["file_bytes"]["quantised_over_bricks"] = round(entry["file_bytes"]["quantised"] / entry["file_bytes"]["bricks"], 4)
        print(f"{res}^3 bytes: {entry['device_bytes']} {entry['file_bytes']}", file=sys.stderr, flush=True)
        entry["codec_seconds"] = {"quantize": round(wall(bricks.quantize), 5), "dequantize": round(wall(q.dequantize), 5)}
        deq = q.dequantize()
        again = deq.quantize()
        entry["quantize_of_dequantize_is_identity"] = bool(torch.equal(again._records, q._records) and torch.equal(again.exponents, q.exponents))
        del again
        variants = {"bricks_default": (bricks, 0)}
        variants.update({f"quantised_lanes_{n}": (q, n) for n in QLANES[args.degree]})
        entry["frame"] = sweep(variants)
        print(f"{res}^3 frame: {entry['frame']}", file=sys.stderr, flush=True)
        # which variant lanes_per_ray=0 picks: the one whose images it reproduces bit for bit
        zero = render(q, *rays[0], lanes_per_ray=0)["image"]
        entry["default_lanes"] = [n for n in QLANES[args.degree] if torch.equal(zero, render(q, *rays[0], lanes_per_ray=n)["image"])]
        same, views, fetched, total = True, [], 0, 0
        for ro, rd in rays:
            a = render(q, ro, rd, lanes_per_ray=1, stats=True)
            b = render(deq, ro, rd, lanes_per_ray=1, stats=True)
            same = same and all(bool(torch.equal(a[k], b[k])) for k in ("image", "depth", "stats"))
            views.append(psnr(render(q, ro, rd)["image"], render(bricks, ro, rd)["image"]))
            st = a["stats"].cpu().numpy()
            fetched += int(st[0]); total += int(st[1])
        entry["lanes_1_bit_identical_to_dequantised"] = same
        entry["fetched"] = round(fetched / max(total, 1), 4)
        entry["psnr_quantised_vs_bricks"] = {"min": round(min(views), 2), "mean": round(float(np.mean(views)), 2)}
        truth = {}
        for name, f in (("bricks", bricks), ("quantised", q)):
            v = [psnr(render(f, ro, rd, outputs="image")["image"], im) for ro, rd, im in held]
            truth[name] = {"min": round(min(v), 3), "mean": round(float(np.mean(v)), 3)}
        entry["psnr_held_out"] = truth
        print(f"{res}^3 psnr: {entry['psnr_quantised_vs_bricks']} {truth}", file=sys.stderr, flush=True)
        return entry

    for res in args.resolutions:
        out[f"{res}^3"] = measure(res)
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
