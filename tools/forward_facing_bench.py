"""Forward-facing scenes: what NDC rays buy, and what the two new ray launches cost.  One GPU, one JSON document
(profiles/forward_facing_bench.json unless --out says otherwise).

The scene is procedural, in the spirit of tests/procedural_scene.py: Gaussian blobs at depths from 2 to 20 in front of a 5 x 5 grid of
cameras that look along -z, and a textured wall at depth 20 behind them, so that every ray ends on something, as in a real
forward-facing capture.  The views are rendered in fp64 (1,024 samples per ray, linear in disparity) and written out as an LLFF
directory -- poses_bounds.npy + images/ -- which the tool then reads back through LLFFDatasetLoader and trains on through
`NeRF.fit(train.ray_batches(...))`, as a user's script would.

  convergence  --seeds fresh models per ray model, the same seeds for every model: "ndc" (NDC rays, samples over the whole ray),
               "linear" (pinhole rays, samples linear in depth over the scene's bounds), "disparity" (pinhole rays, samples linear in
               disparity over the same bounds).  Held-out fine PSNR (`evaluate` on the held-out views) at each step count of --at.
  launches     the two new launches beside the plain ones at 32,768 rays x 64 samples, in the same process: device events around
               --launches back-to-back calls on preallocated outputs, the variants in turn, --repeats rounds; microseconds per launch.

    python tools/forward_facing_bench.py [--at 200,500,1000,2000] [--seeds 2] [--no-convergence] [--no-launches] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, FOCAL, GRID, HOLDOUT = 128, 96, 120.0, 5, 8
RAYS, CHUNK, N_COARSE, STEPS_PER_EPOCH = 32768, 4096, 64, 50
NEAR_DEPTH, WALL_DEPTH, FAR_DEPTH = 1.8, 20.0, 28.0      # the wall lies at distance 20 / cos <= 26 along the outermost rays


def camera_poses():
    """[V,4,4] float64 camera-to-world (right, up, backwards): a GRID x GRID lattice in the plane z = 0, each camera turned a little
    towards the point (0, 0, -6)"""
    import numpy as np
    out = []
    for iy in range(GRID):
        for ix in range(GRID):
            c = np.array([(ix / (GRID - 1) - 0.5) * 1.6, (iy / (GRID - 1) - 0.5) * 1.0, 0.0])
            z = c - np.array([0.0, 0.0, -6.0]); z /= np.linalg.norm(z)
            x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
            m = np.eye(4)
            m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, c
            out.append(m)
    return np.stack(out)


def field(p):
    """analytic scene (torch, fp64): p [...,3] -> sigma [...], rgb [...,3].  Blobs whose size grows with their depth, and a wall"""
    import torch
    blobs = [((-0.5, 0.2, -2.2), 0.25), ((0.6, -0.3, -3.0), 0.3), ((0.0, 0.1, -4.5), 0.45), ((-1.4, -0.6, -6.5), 0.6),
             ((1.6, 0.8, -8.0), 0.7), ((0.3, -1.5, -11.0), 1.0), ((-2.5, 1.6, -14.0), 1.3), ((3.0, -0.5, -17.0), 1.6)]
    sigma = torch.zeros(p.shape[:-1], dtype=p.dtype, device=p.device)
    rgb = torch.zeros_like(p)
    for k, (c, r) in enumerate(blobs):
        d2 = ((p - torch.tensor(c, dtype=p.dtype, device=p.device)) ** 2).sum(-1)
        s = (30.0 / r) * torch.exp(-d2 / (0.5 * r * r))
        col = torch.tensor([0.5 + 0.5 * math.sin(1.7 * k), 0.5 + 0.5 * math.sin(2.9 * k + 1.0), 0.5 + 0.5 * math.sin(4.1 * k + 2.0)],
                           dtype=p.dtype, device=p.device)
        stripes = 0.75 + 0.25 * torch.sin((p[..., 0] + p[..., 1]) * (6.0 / r))
        sigma = sigma + s
        rgb = rgb + s[..., None] * col * stripes[..., None]
    wall = 40.0 * (p[..., 2] < -WALL_DEPTH).to(p.dtype)
    wall_rgb = torch.stack([0.5 + 0.4 * torch.sin(0.9 * p[..., 0]), 0.5 + 0.4 * torch.sin(1.3 * p[..., 1] + 1.0),
                            0.5 + 0.4 * torch.sin(0.7 * (p[..., 0] - p[..., 1]))], -1)
    total = sigma + wall
    rgb = (rgb + wall[..., None] * wall_rgb) / total.clamp(min=1e-12)[..., None]
    return total, rgb.clamp(0, 1)


def write_scene(root):
    """the scene as an LLFF directory: poses_bounds.npy (rotation columns stored as (down, right, backwards), hwf, depth bounds) and
    images/view_XXX.png"""
    import numpy as np
    import torch
    from PIL import Image
    from keras_nerf_amd.runtime import KnerfContext
    poses = camera_poses()
    ctx = KnerfContext()
    o, d, _ = ctx.generate_rays(poses.astype(np.float32), FOCAL, H, W, NEAR_DEPTH, FAR_DEPTH, 2, None)
    ctx.close()
    s = torch.linspace(0.0, 1.0, 1024, device="cuda", dtype=torch.float64)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    rows = []
    for v in range(len(poses)):
        # depth along the view axis -> distance along the ray: samples linear in disparity between the depth bounds
        cosine = (d[v].double() * torch.as_tensor(-poses[v, :3, 2], device="cuda")).sum(-1, keepdim=True)
        tt = (1.0 / ((1.0 - s) / NEAR_DEPTH + s / (FAR_DEPTH + 2.0))) / cosine                   # [H,W,1024]
        img = []
        for r0 in range(0, H, 16):                                                            # rows in slabs: 16 x W x 1024 points
            sl = slice(r0, r0 + 16)
            p = o[v, sl].double()[..., None, :] + d[v, sl].double()[..., None, :] * tt[sl][..., None]
            sg, col = field(p)
            delta = torch.cat([tt[sl][..., 1:] - tt[sl][..., :-1], tt.new_full((*tt[sl].shape[:-1], 1), 1e10)], -1)
            alpha = 1.0 - torch.exp(-sg * delta)
            T = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1.0 - alpha[..., :-1]], -1), -1)
            img.append(((alpha * T)[..., None] * col).sum(-2))
        img = torch.cat(img).clamp(0, 1).cpu().numpy()
        Image.fromarray((img * 255 + 0.5).astype(np.uint8), "RGB").save(os.path.join(root, "images", f"view_{v:03d}.png"))
        R, t = poses[v, :3, :3], poses[v, :3, 3]
        stored = np.stack([-R[:, 1], R[:, 0], R[:, 2], t, np.array([H, W, FOCAL])], -1)
        rows.append(np.concatenate([stored.reshape(-1), [NEAR_DEPTH, FAR_DEPTH]]))
    np.save(os.path.join(root, "poses_bounds.npy"), np.stack(rows))
    return root


def time_launches(n_launches, repeats):
    """microseconds per launch of the plain and the new ray launches at RAYS rays x N_COARSE samples"""
    import numpy as np
    import torch
    from keras_nerf_amd import _lib
    lib = _lib.load()
    V, N = 21, N_COARSE
    g = torch.Generator(device="cuda").manual_seed(0)
    images = torch.rand((V, H, W, 4), device="cuda", generator=g)
    c2w = torch.as_tensor(camera_poses()[:V].astype(np.float32), device="cuda")
    o = torch.empty((RAYS, 3), device="cuda"); d = torch.empty_like(o); tg = torch.empty_like(o); t = torch.empty((RAYS, N), device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, VH, VW = 2, 128, 128                                   # 32,768 rays as two whole views
    models = {"pinhole_linear": _lib.KnerfRayModel(0, 0, 1.0), "ndc": _lib.KnerfRayModel(1, 0, 1.0), "disparity": _lib.KnerfRayModel(0, 1, 1.0)}
    rng = {"pinhole_linear": (2.0, 6.0), "ndc": (0.0, 1.0), "disparity": (2.0, 6.0)}

    def batch(model, k):
        near, far = rng[model] if model else (2.0, 6.0)
        args = (None, stream, p(images), p(c2w), V, H, W, 4, FOCAL, near, far, N, 1, 0, 0, RAYS, None, k, p(o), p(d), p(t), p(tg), None)
        return lib.knerf_draw_ray_batch(*args) if model is None else lib.knerf_draw_ray_batch_ext(*args, C.byref(models[model]))

    def views(model, k):
        near, far = rng[model] if model else (2.0, 6.0)
        args = (None, stream, p(c2w), None, 1, k, B, VH, VW, N, FOCAL, near, far, p(o), p(d), p(t))
        return lib.knerf_generate_rays(*args) if model is None else lib.knerf_generate_rays_ext(*args, C.byref(models[model]))

    variants = [(f"{kind}_{model or 'plain'}", fn, model) for kind, fn in (("ray_batch", batch), ("views", views))
                for model in (None, "pinhole_linear", "ndc", "disparity")]
    spent = {name: [] for name, _, _ in variants}
    for name, fn, model in variants:                          # warm-up: code objects loaded, every shape launched once
        assert fn(model, 0) == 0, name
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn, model in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(n_launches):
                fn(model, k)
            e1.record(); torch.cuda.synchronize()
            spent[name].append(e0.elapsed_time(e1) / n_launches * 1e3)
    return {name: {"us_per_launch": round(float(np.median(v)), 2), "rounds": [round(x, 2) for x in v]} for name, v in spent.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--at", default="200,500,1000,2000", help=f"step counts at which the held-out PSNR is taken (multiples of {STEPS_PER_EPOCH})")
    ap.add_argument("--seeds", type=int, default=2)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-convergence", action="store_true")
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_facing_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd.data.llff import LLFFDatasetLoader
    from keras_nerf_amd.model.nerf.nerf import NeRF

    out = {"tool": "forward_facing_bench", "image_width": W, "image_height": H, "views": GRID * GRID, "holdout": HOLDOUT,
           "rays_per_step": RAYS, "ray_chunks": CHUNK, "samples": [N_COARSE, 128], "device": torch.cuda.get_device_name(0)}
    if not args.no_launches:
        out["launch_rays_x_samples"] = [RAYS, N_COARSE]
        out["launches_timed"] = [args.launches, args.repeats]
        out["launch_us"] = time_launches(args.launches, args.repeats)
        print(json.dumps(out["launch_us"]), file=sys.stderr, flush=True)
    if not args.no_convergence:
        root = write_scene(tempfile.mkdtemp(prefix="knerf_forward_facing_"))
        at = [int(a) for a in args.at.split(",") if a]
        assert all(a % STEPS_PER_EPOCH == 0 for a in at)
        probe = LLFFDatasetLoader(root)
        probe.load_dataset(1, W, H, 0.0, 1.0, N_COARSE)
        near, far = float(probe.bounds.min()), float(probe.bounds.max())            # the scene's bounds in the normalised units
        out["pinhole_near_far"] = [round(near, 4), round(far, 4)]
        modes = {"ndc": dict(ndc=True), "linear": dict(ndc=False, spacing="linear"), "disparity": dict(ndc=False, spacing="disparity")}
        table = {m: [] for m in modes}
        for seed in range(args.seeds):
            for name, kw in modes.items():
                train, _, test = LLFFDatasetLoader(root, holdout=HOLDOUT, **kw).load_dataset(1, W, H, near, far, N_COARSE)
                ds = train.ray_batches(RAYS, seed=seed, steps_per_epoch=STEPS_PER_EPOCH)
                nerf = NeRF(seed=seed)
                nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=1, image_height=H, image_width=W, ray_chunks=CHUNK)
                row, epoch = [], 0
                for a in at:
                    nerf.fit(ds, epochs=a // STEPS_PER_EPOCH, initial_epoch=epoch, verbose=0); epoch = a // STEPS_PER_EPOCH
                    row.append(round(float(nerf.evaluate(test, return_dict=True)["fine_psnr"]), 2))
                table[name].append(row)
                print(f"seed {seed} {name}: held-out fine PSNR {row} at steps {at}", file=sys.stderr, flush=True)
                nerf._ctx.close()
        out["train_views"], out["held_out_views"] = len(train.image_paths), len(test.image_paths)
        out["held_out_fine_psnr_at_steps"] = at
        for name, rows in table.items():
            out[f"{name}_psnr_by_seed"] = rows
            out[f"{name}_psnr_mean"] = [round(float(np.mean(c)), 2) for c in zip(*rows)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
