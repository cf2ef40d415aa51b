"""Early ray termination on a cfg5-shaped sweep, one GPU, one JSON line: 36 poses pose_spherical(theta, -30, 4) at 256 x 256,
ray_chunks 4096, outputs ("image", "depth"), rendered in five modes:
  dense; termination only (set_ray_termination(--threshold)); grid only (build_occupancy_grid(--grid)); grid + termination; and
  termination with an eps that (nearly) never triggers (--never, 1e-30): the cost of the rounds themselves.
Per mode: median frame time (device events around predict_and_render_images), the evaluated fraction of each net (termination_stats;
occupancy_stats for the grid alone), the PSNR of the fine image against the dense frame (min and mean over the sweep).  Then the
termination-only and grid + termination modes again for each segment length of --segments, and termination only for each eps
of --thresholds at each of those lengths.  The same fine-sampler random numbers for every mode (u fixed per pose).

    python tools/termination_bench.py [--train-steps 600] [--threshold 1e-4] [--segments 16,32,64] [--model_dirs coarse.h5,fine.h5]

Without --model_dirs it trains the compact procedural scene (tests/procedural_scene.py) at 128 x 128 for --train-steps steps, as
tools/occupancy_bench.py does; with it, it loads the two Keras .h5 weight files (coarse, fine).
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
    ap.add_argument("--threshold", type=float, default=1e-4)
    ap.add_argument("--never", type=float, default=1e-30)
    ap.add_argument("--segment", type=int, default=32, help="L of the five modes")
    ap.add_argument("--segments", default="16,32,64", help="the L sweep")
    ap.add_argument("--thresholds", default="1e-3,1e-2", help="termination only for each of these eps too, at each L of --segments")
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--model_dirs", default="", help="coarse.h5,fine.h5")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd.data.utils import get_focal_from_fov, pose_spherical
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import FOV, make_scene

    out = {"tool": "termination_bench", "wh": 256, "frames": args.frames, "ray_chunks": 4096, "threshold": args.threshold,
           "segment": args.segment, "grid": args.grid}
    wh = 256
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

    def sweep():
        ms, imgs = [], []
        nerf.predict_and_render_images(rays[0][0], u=rays[0][1], outputs=("image", "depth"))     # warm-up (workspaces)
        torch.cuda.synchronize()
        nerf.termination_stats(reset=True); nerf.occupancy_stats(reset=True)
        for r, u in rays:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, fine = nerf.predict_and_render_images(r, u=u, outputs=("image", "depth"))
            b.record(); b.synchronize()
            ms.append(a.elapsed_time(b))
            imgs.append(fine["image"].clone())
        return float(np.median(ms)), imgs

    def record(name, ms, imgs, stats):
        out[f"{name}_ms"] = round(ms, 3)
        out[f"{name}_vs_dense"] = round(ms / dense_ms, 3)
        if stats is not None:
            out[f"{name}_evaluated"] = {k: round(v[0] / max(v[1], 1), 4) for k, v in stats.items()}
        if imgs is not None:
            psnr = [float(-10 * np.log10(max(float(((a - b) ** 2).mean()), 1e-20))) for a, b in zip(imgs, dense)]
            out[f"{name}_psnr_min"], out[f"{name}_psnr_mean"] = round(min(psnr), 2), round(float(np.mean(psnr)), 2)

    dense_ms, dense = sweep()
    out["dense_ms"] = round(dense_ms, 3)
    nerf.set_ray_termination(args.threshold, args.segment)
    ms, imgs = sweep(); record("term", ms, imgs, nerf.termination_stats())
    nerf.set_ray_termination(args.never)
    ms, imgs = sweep(); record("term_never", ms, imgs, nerf.termination_stats())
    out["term_never_bit_identical"] = all(bool(torch.equal(a, b)) for a, b in zip(imgs, dense))
    nerf.set_ray_termination(0)
    grids = nerf.build_occupancy_grid(args.grid)
    out["occupied_cells"] = {k: round(float(v.mean()), 4) for k, v in grids.items()}
    ms, imgs = sweep(); record("grid", ms, imgs, nerf.occupancy_stats())
    nerf.set_ray_termination(args.threshold, args.segment)
    ms, imgs = sweep(); record("grid_term", ms, imgs, nerf.termination_stats())
    for seg in (int(s) for s in args.segments.split(",") if s):
        nerf.set_ray_termination(args.threshold, seg)
        ms, imgs = sweep(); record(f"grid_term_L{seg}", ms, imgs, nerf.termination_stats())
    nerf.clear_occupancy_grid()
    for seg in (int(s) for s in args.segments.split(",") if s):
        nerf.set_ray_termination(args.threshold, seg)
        ms, imgs = sweep(); record(f"term_L{seg}", ms, imgs, nerf.termination_stats())
    for eps in (float(e) for e in args.thresholds.split(",") if e):
        for seg in (int(s) for s in args.segments.split(",") if s):
            nerf.set_ray_termination(eps, seg)
            ms, imgs = sweep(); record(f"term_eps{eps:g}_L{seg}", ms, imgs, nerf.termination_stats())
    nerf.set_ray_termination(0)
    ms, imgs = sweep(); record("dense_again", ms, None, None)
    out["dense_again_bit_identical"] = all(bool(torch.equal(a, b)) for a, b in zip(imgs, dense))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
