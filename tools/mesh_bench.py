"""Times the trained-field extensions on one GPU and prints one JSON line: the fine MLP on a 256^3 and a 512^3 grid (knerf_query_grid,
sigma only) on the fused kernel and on the general-shape route (KNERF_FLAG_FORCE_GENERIC: positional-encoding op + general MLP in
chunks), and marching cubes (knerf_marching_cubes, count + emit) on the 256^3 / 512^3 grids.  Default network shape, the weights of
tests/problem.py; device events around each call after warm-up, median of --reps.

    python tools/mesh_bench.py [--reps 5] [--sizes 256,512] [--no-general]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()                # warm-up (workspaces, attributes)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--no-general", action="store_true")
    args = ap.parse_args()
    import numpy as np
    from oracle import nerf_oracle as O
    from keras_nerf_amd.runtime import FINE, KnerfContext, marching_cubes
    from tests.problem import make_problem
    P = make_problem(n_images=1, wh=16, weight_scale=1.5, bias_std=0.05)
    lo, hi = (-1.5,) * 3, (1.5,) * 3
    out = {"tool": "mesh_bench", "shape": "8,4,256", "reps": args.reps}
    ctxs = {"fused": KnerfContext()}
    if not args.no_general:
        ctxs["general"] = KnerfContext(force_generic=True)
    for c in ctxs.values():
        c.set_weights(0, O.flatten_params(P["cp"])); c.set_weights(1, O.flatten_params(P["fp"]))
    for r in (int(s) for s in args.sizes.split(",")):
        n = r ** 3
        for name, c in ctxs.items():
            ms = timed(lambda: c.query_grid(FINE, (r, r, r), lo, hi), args.reps)
            out[f"grid{r}_{name}_ms"] = round(ms, 3)
            out[f"grid{r}_{name}_points_per_s"] = float(f"{n / (ms * 1e-3):.4g}")
        sigma, _ = ctxs["fused"].query_grid(FINE, (r, r, r), lo, hi)
        tau = float(np.quantile(sigma[::4, ::4, ::4].cpu().numpy(), 0.7))
        out[f"mc{r}_ms"] = round(timed(lambda: marching_cubes(sigma, tau, lo, hi), args.reps), 3)
        v, f, _ = marching_cubes(sigma, tau, lo, hi)
        out[f"mc{r}_vertices"], out[f"mc{r}_faces"] = int(v.shape[0]), int(f.shape[0])
        del sigma, v, f
    for c in ctxs.values():
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
