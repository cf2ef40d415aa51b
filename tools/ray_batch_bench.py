"""Training on random ray batches against training on whole images, one GPU, one JSON line.

The procedural scene of tests/procedural_scene.py at 128 x 128 (100 training views, 4 held out) is written as a nerf_synthetic-layout
directory and read back through DatasetLoader, so both modes run through `NeRF.fit` as a user's script would: image mode with batch 2
(32,768 rays a step, ray_chunks 4096 -- the configuration of bench.py's default line), ray mode with
`train.ray_batches(32768)`; 50 steps an epoch either way.

  timing       (--timing-scene procedural | discs) one model, dead-tile skipping off (so every step does the same work),
               --warmup-epochs epochs of each mode, then
               --timed-epochs epochs of each mode in turn (image, ray, image, ray, ...), each `fit` call timed from a device
               synchronisation before it to one after it: ms per step of both modes and their ratio.
  convergence  --seeds fresh models per mode; held-out fine PSNR (`evaluate` on the 4 held-out views: the mean of the per-image PSNRs)
               after each step count of --at.

    python tools/ray_batch_bench.py [--timed-epochs 6] [--at 100,300,1000,2000] [--seeds 3] [--no-timing] [--no-convergence]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WH, N_TRAIN, N_HELD, RAYS, CHUNK = 128, 100, 4, 32768, 4096


def write_scene(root):
    """the procedural scene as transforms_{train,val,test}.json + RGBA PNGs (val = test = the held-out views)"""
    import numpy as np
    from PIL import Image
    from keras_nerf_amd.data.utils import pose_spherical
    from keras_nerf_amd.runtime import KnerfContext
    from tests.procedural_scene import FOV, make_scene
    V = N_TRAIN + N_HELD
    ctx = KnerfContext(white_background=True)
    img = make_scene(ctx, wh=WH, n_views=V, scale=1.6)[3].cpu().numpy()
    ctx.close()
    poses = [pose_spherical(360.0 * i / V * 7 % 360.0, -30.0 + 20.0 * np.sin(0.7 * i), 4.0) for i in range(V)]      # make_scene's cameras
    # the held-out views are spread over the orbit: every 26th view
    held = list(range(12, V, V // N_HELD))[:N_HELD]
    split = {"train": [i for i in range(V) if i not in held], "val": held, "test": held}
    for subset, views in split.items():
        os.makedirs(os.path.join(root, subset), exist_ok=True)
        frames = []
        for k, i in enumerate(views):
            rgba = np.concatenate([img[i], np.ones_like(img[i][..., :1])], -1)
            Image.fromarray((rgba * 255 + 0.5).astype(np.uint8), "RGBA").save(os.path.join(root, subset, f"r_{k}.png"))
            frames.append({"file_path": f"./{subset}/r_{k}", "transform_matrix": np.asarray(poses[i]).tolist()})
        json.dump({"camera_angle_x": FOV, "frames": frames}, open(os.path.join(root, f"transforms_{subset}.json"), "w"))
    return root


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup-epochs", type=int, default=1)
    ap.add_argument("--timed-epochs", type=int, default=6, help="per mode; 50 steps each")
    ap.add_argument("--at", default="100,300,1000,2000", help="step counts at which the held-out PSNR is taken (multiples of 50)")
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--timing-scene", default="procedural", choices=["procedural", "discs"],
                    help="discs: time on the dataset of `bench.py --mode fit` (bench.write_synthetic_dataset) instead, to set the ray "
                         "mode beside that line; the step time depends on the images a little even with skipping off")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--no-convergence", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd.data.loader import DatasetLoader
    from keras_nerf_amd.model.nerf.nerf import NeRF

    root = write_scene(tempfile.mkdtemp(prefix="knerf_ray_batch_"))

    def datasets(seed, root=root):
        train, _, test = DatasetLoader(root, white_background=True).load_dataset(2, WH, WH, 2.0, 6.0, 64)
        return train, train.ray_batches(RAYS, seed=seed), test

    def model(seed):
        nerf = NeRF(seed=seed)
        nerf.compile({"learning_rate": 5e-4}, "mse", batch_size=2, image_height=WH, image_width=WH, ray_chunks=CHUNK, white_background=True)
        return nerf

    out = {"tool": "ray_batch_bench", "wh": WH, "train_views": N_TRAIN, "held_out_views": N_HELD, "rays_per_step": RAYS,
           "ray_chunks": CHUNK, "device": torch.cuda.get_device_name(0)}
    if not args.no_timing:
        if args.timing_scene == "discs":
            from bench import write_synthetic_dataset
            image_ds, ray_ds, _ = datasets(0, write_synthetic_dataset(tempfile.mkdtemp(prefix="knerf_ray_batch_discs_"), WH))
        else:
            image_ds, ray_ds, _ = datasets(0)
        out["timing_scene"] = args.timing_scene
        nerf = model(0)
        nerf._ctx.set_option("skip_dead_tiles", 0)
        steps = len(image_ds)
        assert steps == len(ray_ds) == 50
        epoch = 0
        for _ in range(args.warmup_epochs):
            for ds in (image_ds, ray_ds):
                nerf.fit(ds, epochs=epoch + 1, initial_epoch=epoch, verbose=0); epoch += 1
        spent = {"image": [], "ray": []}
        for _ in range(args.timed_epochs):
            for name, ds in (("image", image_ds), ("ray", ray_ds)):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                nerf.fit(ds, epochs=epoch + 1, initial_epoch=epoch, verbose=0); epoch += 1
                torch.cuda.synchronize(); spent[name].append((time.perf_counter() - t0) / steps * 1e3)
        out["timed_steps_per_mode"] = steps * args.timed_epochs
        for name, ms in spent.items():
            out[f"{name}_ms_per_step"] = round(float(np.mean(ms)), 3)
            out[f"{name}_ms_per_step_epochs"] = [round(m, 3) for m in ms]
        out["ray_over_image"] = round(float(np.mean(spent["ray"]) / np.mean(spent["image"])), 4)
        nerf._ctx.close()
    if not args.no_convergence:
        at = [int(a) for a in args.at.split(",") if a]
        assert all(a % 50 == 0 for a in at)
        table = {"image": [], "ray": []}
        for seed in range(args.seeds):
            for name in ("image", "ray"):
                image_ds, ray_ds, test = datasets(seed)
                ds = image_ds if name == "image" else ray_ds
                nerf = model(seed)
                row, epoch = [], 0
                for a in at:
                    nerf.fit(ds, epochs=a // 50, initial_epoch=epoch, verbose=0); epoch = a // 50
                    row.append(round(float(nerf.evaluate(test, return_dict=True)["fine_psnr"]), 2))
                table[name].append(row)
                print(f"seed {seed} {name} mode: held-out fine PSNR {row} at steps {at}", file=sys.stderr, flush=True)
                nerf._ctx.close()
        out["held_out_fine_psnr_at_steps"] = at
        for name, rows in table.items():
            out[f"{name}_psnr_by_seed"] = rows
            out[f"{name}_psnr_mean"] = [round(float(np.mean(c)), 2) for c in zip(*rows)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
