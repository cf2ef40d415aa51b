"""Point queries, density grids and mesh export of baked fields against the MLP they were baked from, one GPU, one JSON document
(profiles/baked_query_bench.json with --out).  Protocol of tools/baked_bench.py: the compact procedural scene (40 views, 128 x 128)
trained for --train-steps steps and baked at degree --degree on --resolution^3 over the default box.  For the dense BakedField, its
BrickBakedField (bricks of --brick^3) and its QuantizedBrickField, each figure the median of --repeat HIP-event timings after a warm-up
call, with the spread (max - min) beside it:
  - density_grid() on the lattice itself (the stored sigma column, no kernel of csrc/baked_query.hip);
  - density_grid on a foreign grid of the same size (another box: the sigma-only kernel in grid mode, no coordinate tensor);
  - query of --points random points inside the box with per-point directions, at one lane per point and at the group variant,
    and which of the two lanes_per_point=0 picks;
  - the sigma-only query of the same points;
  - extract_mesh at --threshold without and with vertex colours, and the mesh's size;
  - NeRF.density_grid(resolution) and NeRF.extract_mesh of the MLP, for comparison.

    python tools/baked_mesh_bench.py [--train-steps 600] [--resolution 256] [--points 1000000] [--out profiles/baked_query_bench.json]
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
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--brick", type=int, default=8)
    ap.add_argument("--sigma-threshold", type=float, default=1.0, help="densities at or below it are baked as empty")
    ap.add_argument("--threshold", type=float, default=10.0, help="the density the mesh is extracted at")
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd import baked_query
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import make_scene

    tw, batch, n_train = 128, 2, 40
    R = args.resolution
    out = {"tool": "baked_mesh_bench", "resolution": R, "degree": args.degree, "brick": args.brick, "points": args.points,
           "sigma_threshold": args.sigma_threshold, "mesh_threshold": args.threshold, "repeat": args.repeat,
           "device": torch.cuda.get_device_name(0)}
    c0 = KnerfContext(white_background=True)
    o, d, t, img = make_scene(c0, wh=tw, n_views=n_train, scale=1.6, compact=True)
    c0.close()
    nerf = NeRF(seed=0)
    nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=batch, image_height=tw, image_width=tw, ray_chunks=4096, white_background=True)
    order = np.random.default_rng(5).integers(0, n_train, (args.train_steps, batch))
    t0 = time.time()
    for s in range(args.train_steps):
        idx = torch.as_tensor(order[s], device="cuda")
        nerf.train_step((img[idx], (o[idx], d[idx], t[idx])), with_metrics=False)
    nerf._ctx.poll_nonfinite(wait=True)
    out["train"] = f"compact procedural scene, {tw}x{tw}, batch {batch}, {args.train_steps} steps on {n_train} views ({time.time() - t0:.1f} s)"
    del o, d, t, img

    def timed(fn):
        """milliseconds: the median of --repeat HIP-event timings after a warm-up call, and their spread"""
        fn()
        ms = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = fn()
            b.record(); b.synchronize()
            ms.append(a.elapsed_time(b))
            del r
        return {"ms": round(float(np.median(ms)), 4), "spread_ms": round(max(ms) - min(ms), 4)}

    dense = nerf.bake(resolution=R, sh_degree=args.degree, sigma_threshold=args.sigma_threshold)
    bricks = dense.compact(args.brick)
    fields = {"dense": dense, "bricks": bricks, "quantised": bricks.quantize()}
    lo, hi = dense.bounds
    foreign = (tuple(v - 0.13 for v in lo), tuple(v + 0.07 for v in hi))
    rng = np.random.default_rng(11)
    pts = torch.as_tensor(rng.uniform(lo, hi, (args.points, 3)).astype(np.float32)).cuda()
    dirs = torch.as_tensor(rng.normal(size=(args.points, 3)).astype(np.float32)).cuda()
    out["n_bricks"] = bricks.n_bricks
    for name, f in fields.items():
        e = {"density_grid_lattice": timed(lambda: f.density_grid()),
             "density_grid_foreign": timed(lambda: f.density_grid(R, foreign))}
        lanes = baked_query._storage(f)[1]
        for n in lanes:
            e[f"query_lanes_{n}"] = timed(lambda: f.query(pts, dirs, lanes_per_point=n))
        zero = f.query(pts[:4096], dirs[:4096])[0]
        e["default_lanes"] = [n for n in lanes if torch.equal(zero, f.query(pts[:4096], dirs[:4096], lanes_per_point=n)[0])]
        e["query_sigma_only"] = timed(lambda: baked_query.query_sigma(f, pts))
        e["query_with_gradient"] = timed(lambda: f.query(pts, dirs, gradient=True))
        e["extract_mesh"] = timed(lambda: f.extract_mesh(args.threshold))
        e["extract_mesh_vertex_colors"] = timed(lambda: f.extract_mesh(args.threshold, vertex_colors=True))
        v, t3, _ = f.extract_mesh(args.threshold)
        e["mesh"] = {"vertices": int(v.shape[0]), "faces": int(t3.shape[0])}
        out[name] = e
        print(f"{name}: {e}", file=sys.stderr, flush=True)
    m = {"density_grid": timed(lambda: nerf.density_grid(R, (lo, hi))),
         "extract_mesh": timed(lambda: nerf.extract_mesh(args.threshold, R, (lo, hi))),
         "extract_mesh_vertex_colors": timed(lambda: nerf.extract_mesh(args.threshold, R, (lo, hi), vertex_colors=True))}
    v, t3, _ = nerf.extract_mesh(args.threshold, R, (lo, hi))
    m["mesh"] = {"vertices": int(v.shape[0]), "faces": int(t3.shape[0])}
    out["mlp"] = m
    print(f"mlp: {m}", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
