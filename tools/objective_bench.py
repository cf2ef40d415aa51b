"""What the extended objective costs: the cfg2 train step of bench.py (128 x 128, batch 2, ray_chunks 4096, coarse 64 + fine 128) under the
plain objective, each loss kind, each regulariser and everything together (knerf_set_objective; csrc/composite_ext.hip).  Per mode the
median step time over --steps steps after --warmup, in milliseconds, its difference to plain, and the compositing kernels' own time
per pass from the library's HIP-event profile (knerf_profile_read, class "composite": compositing + its loss / term reductions) over
two further steps.  One JSON file under profiles/ (and the same as one line on stdout).

    python tools/objective_bench.py [--steps 30] [--warmup 5] [--repeats 3] [--out profiles/objective_bench_cfg2.json]

--repeats: the modes are run round-robin that many times (machines differ by a few per cent from run to run); per mode the median of the
repeats' medians is reported with their min and max.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", default="", help="comma-separated subset of the modes (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective_bench_cfg2.json"))
    args = ap.parse_args()
    import torch
    import bench
    from keras_nerf_amd import _lib, losses
    from keras_nerf_amd.model.nerf.nerf import NeRF

    wh, batch, chunks, desc = bench.CONFIGS["cfg2"]
    R = losses.RayRegularizers
    modes = [("plain", "mse", None), ("mae", "mae", None), ("huber", losses.Huber(0.25), None), ("log_cosh", "log_cosh", None),
             ("distortion", "mse", R(distortion=0.01)), ("opacity_entropy", "mse", R(opacity_entropy=0.001)),
             ("all", losses.Huber(0.25), R(distortion=0.01, opacity_entropy=0.001))]
    if args.modes:
        modes = [m for m in modes if m[0] in args.modes.split(",")]
    out = {"tool": "objective_bench", "config": desc, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "build": _lib.build_info(), "modes": {}}
    runs = {name: [] for name, _, _ in modes}
    comp = {name: [] for name, _, _ in modes}
    for _ in range(args.repeats):
        for name, loss, reg in modes:
            nerf = NeRF(seed=0)
            nerf.compile(optimizer="adam", loss=loss, regularizers=reg, batch_size=batch, image_height=wh, image_width=wh, ray_chunks=chunks,
                         white_background=True)
            try:
                data = bench.make_batch(nerf, wh, batch, 0)
                ms = []
                for i in range(args.warmup + args.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    nerf.train_step(data, with_metrics=False, sync=False)
                    e1.record()
                    e1.synchronize()
                    if i >= args.warmup:
                        ms.append(e0.elapsed_time(e1))
                ms.sort()
                runs[name].append(ms[len(ms) // 2])
                nerf._ctx.profile_enable(True); nerf._ctx.profile_read()
                for _k in range(2):
                    nerf.train_step(data, with_metrics=False, sync=False)
                torch.cuda.synchronize()
                total, launches = nerf._ctx.profile_read()["composite"]
                nerf._ctx.profile_enable(False)
                comp[name].append(total / max(launches, 1))
                nerf._ctx.poll_nonfinite(wait=True)
            finally:
                nerf._ctx.close()
    med = lambda v: sorted(v)[len(v) // 2]
    for name, _, _ in modes:
        out["modes"][name] = {"step_ms": med(runs[name]), "step_ms_min": min(runs[name]), "step_ms_max": max(runs[name]),
                              "composite_ms_per_pass": med(comp[name])}
    if "plain" in out["modes"]:
        base = out["modes"]["plain"]
        for r in out["modes"].values():
            r["step_over_plain_ms"] = r["step_ms"] - base["step_ms"]
            r["composite_over_plain_ms_per_pass"] = r["composite_ms_per_pass"] - base["composite_ms_per_pass"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
