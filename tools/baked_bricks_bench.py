"""The baked field as sparse bricks against the dense table, one GPU, one JSON document (profiles/baked_bricks_bench.json with --out).
Scene and protocol of tools/baked_bench.py: the compact procedural scene trained for --train-steps steps, baked at 256^3, degree 2,
256 x 256 views on poses pose_spherical(theta, -30, 4), white background, termination --threshold, step = half a cell.  For the dense
BakedField and for BrickBakedField with bricks of 4^3 and 8^3:
  - bytes on the device (records + brick table + bits) and in the saved file;
  - stored bricks over all bricks, and the share of the stored records that are touched (a corner of an occupied cell);
  - NeRF.bake seconds (device-synchronised wall clock, after one warm-up bake), dense / bricks=4 / bricks=8, and compact() seconds;
  - frame time: HIP events around render(), --frames poses per round, the three fields alternating in rotating order inside every
    pose, after a warm-up render of each; the median per round, --rounds rounds, and the spread of the rounds' medians (max - min):
    the run-to-run figure a difference between brick sizes has to exceed;
  - whether the brick images are bit-identical to the dense ones, and the fraction of samples fetched;
  - one 512^3 line (bricks of 8^3 baked directly; the dense table too if the device has room for it).

    python tools/baked_bricks_bench.py [--train-steps 600] [--frames 20] [--rounds 5] [--out profiles/baked_bricks_bench.json]
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
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big", type=int, default=512, help="resolution of the extra line (0: none)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd.baked import BRICKS
    from keras_nerf_amd.data.utils import get_focal_from_fov, pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import FOV, make_scene

    wh = 256
    out = {"tool": "baked_bricks_bench", "wh": wh, "frames": args.frames, "rounds": args.rounds, "threshold": args.threshold,
           "sigma_threshold": args.sigma_threshold, "degree": args.degree, "device": torch.cuda.get_device_name(0)}
    tw, batch = 128, 2
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=tw, n_views=40, scale=1.6, compact=True)
    c0.close()
    trainer = NeRF(seed=0)
    trainer.compile({"learning_rate": 5e-4}, "mse", batch_size=batch, image_height=tw, image_width=tw, ray_chunks=4096, white_background=True)
    order = np.random.default_rng(5).integers(0, 40, (args.train_steps, batch))
    t0 = time.time()
    for s in range(args.train_steps):
        idx = torch.as_tensor(order[s], device="cuda")
        trainer.train_step((img[idx], (o[idx], d[idx], t[idx])), with_metrics=False)
    trainer._ctx.poll_nonfinite(wait=True)
    out["train"] = f"compact procedural scene, {tw}x{tw}, batch {batch}, {args.train_steps} steps ({time.time() - t0:.1f} s)"
    del o, d, t, img
    nerf = NeRF(seed=0)
    nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=1, image_height=wh, image_width=wh, ray_chunks=4096, white_background=True)
    nerf.coarse.set_flat_weights(trainer.coarse.get_flat_weights()); nerf.fine.set_flat_weights(trainer.fine.get_flat_weights())
    trainer._ctx.close()

    focal = get_focal_from_fov(FOV, wh)
    rays = []
    for i in range(args.frames):
        c2w = pose_spherical(360.0 * i / args.frames, -30.0, 4.0)
        o, d, _ = nerf._ctx.generate_rays(np.asarray(c2w, np.float32), focal, wh, wh, 2.0, 6.0, 64, None, seed=i)
        rays.append((o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()))

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.time()
        r = fn()
        torch.cuda.synchronize()
        return time.time() - t0, r

    def render(field, o, d, **kw):
        return field.render(o, d, 2.0, 6.0, white_background=True, termination=args.threshold, outputs=("image", "depth"), **kw)

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

    def storage(field, dense_points):
        occ = field.occupied
        touched = torch.zeros(field.resolution, device=occ.device, dtype=torch.bool)
        cx, cy, cz = occ.shape
        for i in (0, 1):
            for j in (0, 1):
                for k in (0, 1):
                    touched[i:i + cx, j:j + cy, k:k + cz] |= occ
        n_touched = int(touched.sum())
        e = {"occupied_cells": round(float(occ.float().mean()), 4), "touched_points": n_touched}
        if hasattr(field, "brick"):
            stored = field.n_bricks * field.brick ** 3
            e.update(device_bytes=field.nbytes, n_bricks=field.n_bricks, all_bricks=int(field.brick_of.numel()),
                     stored_bricks_share=round(field.n_bricks / field.brick_of.numel(), 4), stored_records=stored,
                     touched_share_of_stored=round(n_touched / stored, 4), records_vs_dense=round(stored / dense_points, 4))
        else:
            e.update(device_bytes=int(field._records.numel() + 4 * field._words.numel()), stored_records=dense_points,
                     touched_share_of_stored=round(n_touched / dense_points, 4))
        return e

    def sweep(fields):
        """frame times per field: rounds x frames, the fields alternating in rotating order inside every pose"""
        names = list(fields)
        for n in names:
            render(fields[n], *rays[0]); render(fields[n], *rays[0])                      # warm-up
        medians = {n: [] for n in names}
        for _ in range(args.rounds):
            ms = {n: [] for n in names}
            for i, (o, d) in enumerate(rays):
                for j in range(len(names)):
                    n = names[(i + j) % len(names)]
                    ms[n].append(timed(lambda: render(fields[n], o, d)))
            for n in names:
                medians[n].append(float(np.median(ms[n])))
        res = {}
        for n in names:
            m = medians[n]
            res[n] = {"ms": round(float(np.median(m)), 4), "round_medians_ms": [round(v, 4) for v in m],
                      "spread_ms": round(max(m) - min(m), 4)}
        return res

    def identical(fields):
        ref, same, frac = None, {}, {}
        for n, f in fields.items():
            imgs, fetched, total = [], 0, 0
            for o, d in rays:
                r = render(f, o, d, stats=True)
                imgs.append((r["image"], r["depth"]))
                st = r["stats"].cpu().numpy()
                fetched += int(st[0]); total += int(st[1])
            frac[n] = round(fetched / max(total, 1), 4)
            if ref is None:
                ref = imgs
            else:
                same[n] = all(bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])) for a, b in zip(ref, imgs))
        return same, frac

    def measure(res, with_dense=True, save_dense=True):
        kw = dict(resolution=res, sh_degree=args.degree, sigma_threshold=args.sigma_threshold)
        entry, fields = {"bake_seconds": {}, "storage": {}}, {}
        points = res ** 3
        if with_dense:
            nerf.bake(**kw)                                                                # warm-up: workspaces, allocator
            entry["bake_seconds"]["dense"], fields["dense"] = wall(lambda: nerf.bake(**kw))
            entry["compact_seconds"] = {}
        for b in BRICKS:
            sec, fields[f"brick_{b}"] = wall(lambda: nerf.bake(bricks=b, **kw))
            sec, fields[f"brick_{b}"] = wall(lambda: nerf.bake(bricks=b, **kw))
            entry["bake_seconds"][f"brick_{b}"] = sec
            if with_dense:
                entry["compact_seconds"][f"brick_{b}"], c = wall(lambda: fields["dense"].compact(b))
                entry.setdefault("bake_equals_compact", {})[f"brick_{b}"] = bool(
                    torch.equal(c._records, fields[f"brick_{b}"]._records) and torch.equal(c.brick_of, fields[f"brick_{b}"].brick_of))
                del c
        entry["bake_seconds"] = {k: round(v, 3) for k, v in entry["bake_seconds"].items()}
        if with_dense:
            entry["compact_seconds"] = {k: round(v, 3) for k, v in entry["compact_seconds"].items()}
        for n, f in fields.items():
            entry["storage"][n] = storage(f, points)
            # (the dense table of the extra line is not written out: its file is its records, bits and a few hundred bytes)
            entry["storage"][n]["file_bytes"] = file_bytes(f) if save_dense or n != "dense" else None
            print(f"{res}^3 {n}: {entry['storage'][n]}", file=sys.stderr, flush=True)
        entry["step"] = 0.5 * float(min(next(iter(fields.values())).cell_size))
        entry["frame"] = sweep(fields)
        print(f"{res}^3 frame: {entry['frame']}", file=sys.stderr, flush=True)
        entry["bit_identical_to_first"], entry["fetched"] = identical(fields)
        return entry

    out[f"{args.resolution}^3"] = measure(args.resolution)
    if args.big:
        try:
            out[f"{args.big}^3"] = measure(args.big, save_dense=False)
        except torch.cuda.OutOfMemoryError as e:
            out[f"{args.big}^3"] = {"dense": f"out of memory ({e})"}
            torch.cuda.empty_cache()
            out[f"{args.big}^3 bricks only"] = measure(args.big, with_dense=False)
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
