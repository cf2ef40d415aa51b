"""What the optimizer extensions cost: knerf_apply_adam at the default shape (595,844 parameters per net), timed with HIP events around
each call, in every mode of knerf_set_optimizer -- plain, each schedule kind, each clip kind, weight decay, and everything together.
Per mode the median of --calls calls after --warmup (200 after 20), in milliseconds, and the difference to plain.  One JSON file under
profiles/ (and the same as one line on stdout).

    python tools/optimizer_bench.py [--calls 200] [--warmup 20] [--out profiles/optimizer_bench.json]

The gradient is refilled from a device copy before every call, outside the timed stretch (apply_adam zeroes the accumulator); its values
are those of tests/adam_reference.gradient_schedule, so the clip thresholds of tests/optimizer_ext_reference.py always clip.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from keras_nerf_amd import _lib
    from keras_nerf_amd import optimizers as K
    from keras_nerf_amd.runtime import KnerfContext
    from tests import adam_reference as A

    sched = {"exponential": K.ExponentialDecay(1e-3, 1000, 0.5), "exponential_staircase": K.ExponentialDecay(1e-3, 1000, 0.5, staircase=True),
             "cosine": K.CosineDecay(1e-3, 1000, alpha=0.1),
             "piecewise": K.PiecewiseConstantDecay([10 * (i + 1) for i in range(15)], [1e-3 * 0.9 ** i for i in range(16)])}
    modes = [("plain", None)]
    modes += [(name, K.OptimizerSpec(schedule=s)) for name, s in sched.items()]
    modes += [("clipvalue", K.OptimizerSpec(clip="clipvalue", clip_arg=1e-3)), ("clipnorm", K.OptimizerSpec(clip="clipnorm", clip_arg=1e-2)),
              ("global_clipnorm", K.OptimizerSpec(clip="global_clipnorm", clip_arg=1.0)), ("weight_decay", K.OptimizerSpec(weight_decay=4e-3)),
              ("all", K.OptimizerSpec(schedule=sched["cosine"], clip="global_clipnorm", clip_arg=1.0, weight_decay=4e-3))]
    out = {"tool": "optimizer_bench", "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "build": _lib.build_info(), "modes": {}}
    for name, spec in modes:
        ctx = KnerfContext(white_background=True)
        try:
            n = ctx.param_count
            for net in (0, 1):
                ctx.set_weights(net, A.start_weights(n, A.W0_SEEDS[net]))
            g = torch.from_numpy(np.concatenate([A.gradient_schedule(n, 1, 11)[0][0], A.gradient_schedule(n, 1, 12)[0][0]])).to(ctx.device)
            if spec is not None:
                ctx.set_optimizer(spec)
            grads = ctx.grads_view()
            ms = []
            for i in range(args.warmup + args.calls):
                grads.copy_(g)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.apply_adam(check=False)
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    ms.append(e0.elapsed_time(e1))
            ctx.poll_nonfinite(wait=True)
            assert ctx.step == args.warmup + args.calls
            ms.sort()
            out["modes"][name] = {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "p90_ms": ms[int(len(ms) * 0.9)]}
        finally:
            ctx.close()
    base = out["modes"]["plain"]["median_ms"]
    for name, r in out["modes"].items():
        r["over_plain_ms"] = r["median_ms"] - base
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
