"""References for the optimizer extensions (csrc/optim_ext.hip, include/knerf.h knerf_set_optimizer): learning-rate schedules, gradient
clipping and decoupled weight decay around the Keras-form Adam of tests/adam_reference.py.

As there: a float64 reference of the whole update, float32 mirrors in the kernel's operation order (they MEASURE what fp32 arithmetic
alone costs on a given input; they are no pass criterion), the cases, and a list of deliberate mistakes.  tests/test_optimizer_ext_host.py
proves on the CPU what the tolerances of tests/test_gpu_optimizer_ext.py rest on; both take inputs, cases and tolerances from here.
Inputs (start weights, gradient schedules, the step-count cases) and the two factors come from tests/adam_reference.py unchanged.

Both nets go through one call: the reference has one optimizer per net (keras_nerf/model/nerf/nerf.py:163-165), so every norm is a
norm of ONE net -- and one of the mistakes below takes it over both."""
import math

import numpy as np

from keras_nerf_amd.model.nerf.mlp import layer_shapes
from tests import adam_reference as A

F32 = np.float32
TOL_FACTOR, POWER_FACTOR = A.TOL_FACTOR, A.POWER_FACTOR
HYPER = A.HYPER["default"]              # (lr, beta1, beta2, epsilon); lr is the constant rate of the cases without a schedule
K_STEPS = 12

# ---- shapes ----------------------------------------------------------------------------------------------------------------------
SHAPES = {
    "default": dict(n_layers=8, dense_units=256, skip_layer=4),        # 595,844 parameters: the last workgroup is partial
    "4x64": dict(n_layers=4, dense_units=64, skip_layer=2),            # small, unaligned tensors
    "4x48": dict(n_layers=4, dense_units=48, skip_layer=2),            # zero-padded to 64 on the device; the references see the real widths
}


def tensor_offsets(n_layers=8, dense_units=256, skip_layer=4, pos_emb_xyz=10, pos_emb_dir=4):
    """n_tensors + 1 ascending offsets of the 2 n_layers + 8 tensors of one net in the flat Keras order"""
    off = [0]
    for _, fi, fo in layer_shapes(n_layers, dense_units, skip_layer, 3 + 6 * pos_emb_xyz, 3 + 6 * pos_emb_dir):
        off += [off[-1] + fi * fo, off[-1] + fi * fo + fo]
    return np.asarray(off, dtype=np.int64)


# ---- schedules -------------------------------------------------------------------------------------------------------------------
def constant(lr):
    return dict(kind="constant", lr=lr)


SCHEDULES = {
    "exp": dict(kind="exponential", lr=1e-3, decay_steps=4, rate=0.5, staircase=False),
    "exp_stair": dict(kind="exponential", lr=1e-3, decay_steps=4, rate=0.5, staircase=True),
    "cosine": dict(kind="cosine", lr=1e-3, decay_steps=8, alpha=0.1),              # four of the twelve steps lie behind the clamp
    "piecewise": dict(kind="piecewise", boundaries=(3, 7), values=(1e-3, 5e-4, 1e-4)),
    "piecewise_zero": dict(kind="piecewise", boundaries=(3, 7), values=(1e-3, 5e-4, 0.0)),
}


def schedule_lr(s, step, mutant=None):
    """lr(step) in Python floats: the formulas of include/knerf.h, restated"""
    kind = s["kind"]
    if kind == "constant":
        return float(s["lr"])
    if kind == "exponential":
        p = step / s["decay_steps"]
        if s["staircase"] and mutant != "staircase_ignored":
            p = math.floor(p)
        return s["lr"] * s["rate"] ** p
    if kind == "cosine":
        c = step if mutant == "cosine_unclamped" else min(step, s["decay_steps"])
        alpha = 0.0 if mutant == "alpha_dropped" else s["alpha"]
        return s["lr"] * ((1.0 - alpha) * (0.5 * (1.0 + math.cos(math.pi * c / s["decay_steps"]))) + alpha)
    if kind == "piecewise":
        for b, v in zip(s["boundaries"], s["values"]):
            if (step < b) if mutant == "piecewise_lt" else (step <= b):
                return float(v)
        return float(s["values"][-1])
    raise ValueError(kind)


def schedule_object(s):
    """the same schedule as a keras_nerf_amd.optimizers object (None: constant)"""
    from keras_nerf_amd import optimizers as K
    if s["kind"] == "constant":
        return None
    if s["kind"] == "exponential":
        return K.ExponentialDecay(s["lr"], s["decay_steps"], s["rate"], staircase=s["staircase"])
    if s["kind"] == "cosine":
        return K.CosineDecay(s["lr"], s["decay_steps"], alpha=s["alpha"])
    return K.PiecewiseConstantDecay(list(s["boundaries"]), list(s["values"]))


# ---- cases -----------------------------------------------------------------------------------------------------------------------
# name -> (base case of adam_reference.CASES: steps, t0, skipped steps and the gradient schedule; schedule; clip (kind, c) or None;
#          weight decay; large: 1,000 entries of +-1e18 in the largest tensor at every step)
CLIP_ALWAYS = {"clipvalue": 1e-3, "clipnorm": 1e-2, "global_clipnorm": 1.0}          # below the values / norms of every step
CLIP_NEVER = {"clipvalue": 1e30, "clipnorm": 1e30, "global_clipnorm": 1e30}          # above any finite fp32 norm of these sizes
WD = 0.5
LARGE_COUNT, LARGE_VALUE = 1000, 1e18


def _case(base="trajectory", sched=None, clip=None, wd=0.0, large=False):
    return dict(base=base, sched=constant(HYPER[0]) if sched is None else SCHEDULES[sched], clip=clip, wd=wd, large=large)


CASES = {
    "exp": _case(sched="exp"),
    "exp_stair": _case(sched="exp_stair"),
    "cosine": _case(sched="cosine"),
    "piecewise": _case(sched="piecewise"),
    "exp_skipped": _case(base="skipped", sched="exp"),
    "exp_resume": _case(base="resume", sched="exp"),
    "clipvalue": _case(clip=("clipvalue", CLIP_ALWAYS["clipvalue"])),
    "clipnorm": _case(clip=("clipnorm", CLIP_ALWAYS["clipnorm"])),
    "global_clipnorm": _case(clip=("global_clipnorm", CLIP_ALWAYS["global_clipnorm"])),
    "clipnorm_large": _case(clip=("clipnorm", CLIP_ALWAYS["clipnorm"]), large=True),
    "global_clipnorm_large": _case(clip=("global_clipnorm", CLIP_ALWAYS["global_clipnorm"]), large=True),
    "decay": _case(wd=WD),
    "all": _case(base="skipped", sched="exp", clip=("global_clipnorm", CLIP_ALWAYS["global_clipnorm"]), wd=WD),
}
SCHEDULE_CASES = ("exp", "exp_stair", "cosine", "piecewise", "exp_skipped", "exp_resume")
CLIP_CASES = ("clipvalue", "clipnorm", "global_clipnorm", "clipnorm_large", "global_clipnorm_large")
DECAY_CASES = ("decay", "all")
GENERIC_CASES = ("global_clipnorm", "decay")          # the forced general-shape context (default shape): one clip case, one decay case
# what the GPU file runs against float64: every case at every shape, and the two above on the general-shape kernels
GPU_RUNS = [(shape, case) for shape in SHAPES for case in CASES]


def case_inputs(case, shape):
    """per net (w0, gradients, classes), then t0, skip, offsets -- exactly what the GPU test injects"""
    c = CASES[case]
    off = tensor_offsets(**SHAPES[shape])
    n = int(off[-1])
    K, t0, skip = A.CASES[c["base"]]
    nets = []
    for net in (0, 1):
        w0, G, cls, _, _ = A.case_inputs(c["base"], net, n)
        if c["large"]:
            t = int(np.argmax(np.diff(off)))                   # the largest tensor
            idx = off[t] + np.arange(LARGE_COUNT) * ((off[t + 1] - off[t]) // LARGE_COUNT)
            G = [g.copy() for g in G]
            cls = cls.copy()
            cls[idx] = A.FREE                                   # (no longer always zero, whatever class they had)
            for k, g in enumerate(G):
                g[idx] = np.where((np.arange(LARGE_COUNT) + k + net) % 2, LARGE_VALUE, -LARGE_VALUE).astype(F32)
        nets.append((w0, G, cls))
    return nets, t0, skip, off


# ---- deliberate mistakes ---------------------------------------------------------------------------------------------------------
MUTANTS = ("schedule_at_t", "staircase_ignored", "cosine_unclamped", "alpha_dropped", "piecewise_lt", "skip_advances_schedule",
           "global_norm_over_both_nets", "norms_swapped", "norm_without_root", "clip_on_m", "clipvalue_one_sided", "sumsq_fp32",
           "decay_with_lr_t", "decay_coupled_l2", "decay_on_skipped_step")


def mutants_for(case):
    """the mistakes that CAN differ on a case"""
    c = CASES[case]
    s, clip, skip = c["sched"], c["clip"], A.CASES[c["base"]][2]
    out = []
    if s["kind"] != "constant":
        out.append("schedule_at_t")
        if skip:
            out.append("skip_advances_schedule")
    if s["kind"] == "exponential" and s["staircase"]:
        out.append("staircase_ignored")
    if s["kind"] == "cosine":
        out += ["cosine_unclamped", "alpha_dropped"]
    if s["kind"] == "piecewise":
        out.append("piecewise_lt")
    if clip is not None:
        out.append("clip_on_m")
        if clip[0] == "clipvalue":
            out.append("clipvalue_one_sided")
        else:
            out += ["norms_swapped", "norm_without_root"]
            if clip[0] == "global_clipnorm":
                out.append("global_norm_over_both_nets")
            if c["large"]:
                out.append("sumsq_fp32")          # (without the large entries an fp32 sum is merely a little less exact)
    if c["wd"] > 0:
        out += ["decay_with_lr_t", "decay_coupled_l2"]
        if skip:
            out.append("decay_on_skipped_step")
    return tuple(out)


# ---- the update ------------------------------------------------------------------------------------------------------------------
def _sumsq(gs, off, dtype=np.float64):
    """per net the per-tensor sums of squares"""
    with np.errstate(over="ignore"):
        return [np.add.reduceat(np.square(g.astype(dtype), dtype=dtype), off[:-1], dtype=dtype) for g in gs]


def _clip_factors(gs, off, clip, mutant=None, dtype=np.float64):
    """per net the factor per ELEMENT for the two norm kinds, in `dtype`"""
    kind, c = clip
    if mutant == "norms_swapped":
        kind = "clipnorm" if kind == "global_clipnorm" else "global_clipnorm"
    ssq = _sumsq(gs, off, F32 if mutant == "sumsq_fp32" else np.float64)
    root = (lambda x: x) if mutant == "norm_without_root" else np.sqrt
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for net, q in enumerate(ssq):
            if kind == "clipnorm":
                f = c / np.maximum(root(q.astype(np.float64)), c)
                out.append(np.repeat(f, np.diff(off)).astype(dtype))
            else:
                tot = float(sum(float(x.astype(np.float64).sum()) for x in ssq)) if mutant == "global_norm_over_both_nets" else float(q.astype(np.float64).sum())
                norm = float(root(tot))
                out.append(np.asarray(c / norm if norm > c else 1.0).astype(dtype))
    return out


def _clip(gs, off, clip, mutant, dtype):
    kind, c = clip
    if kind == "clipvalue":
        cc = dtype(c)
        if mutant == "clipvalue_one_sided":
            return [np.minimum(g, cc) for g in gs]
        return [np.minimum(np.maximum(g, -cc), cc) for g in gs]
    return [g * f for g, f in zip(gs, _clip_factors(gs, off, clip, mutant, dtype))]


def update(case, nets, t0, skip, off, dtype=np.float64, form="kernel", hyper_f32=False, mutant=None, hyper=HYPER):
    """The extended update of both nets over the case's steps: the list, per step, of [weights of the coarse net, of the fine net].
    dtype float64: the reference (mutant: one deliberate mistake).  dtype float32: a mirror, one rounding per operation in the order
    of adam_ext_kernel (form "kernel") or with Keras' b m + (1 - b) g (form "keras"); the rates and the clip factor come from double
    and are rounded once, as on the device; hyper_f32: beta1 / beta2 (and a constant rate) as the float32 the C ABI holds."""
    c = CASES[case]
    sched, clip, wd = c["sched"], c["clip"], c["wd"]
    _, b1, b2, eps = hyper
    h1, h2 = (float(F32(b1)), float(F32(b2))) if hyper_f32 else (b1, b2)
    if hyper_f32 and sched["kind"] == "constant":
        sched = constant(float(F32(sched["lr"])))
    f64 = dtype == np.float64
    W = [np.asarray(w0, dtype=dtype).copy() for w0, _, _ in nets]
    M = [np.zeros_like(w) for w in W]
    V = [np.zeros_like(w) for w in W]
    one = dtype(1)
    applied, sched_step = t0, t0
    out = []
    for k in range(len(nets[0][1])):
        if k in skip:
            if mutant == "skip_advances_schedule":
                sched_step += 1
            if mutant == "decay_on_skipped_step":
                d = dtype(wd * schedule_lr(sched, sched_step))
                W = [w - w * d for w in W]
            out.append([w.copy() for w in W])
            continue
        t = applied + 1
        lr = schedule_lr(sched, sched_step + (1 if mutant == "schedule_at_t" else 0), mutant)
        lr_t = dtype(lr * math.sqrt(1 - h2 ** t) / (1 - h1 ** t))
        gs = [np.asarray(G[k], dtype=dtype) for _, G, _ in nets]
        if clip is not None and mutant != "clip_on_m":
            gs = _clip(gs, off, clip, mutant, dtype)
        if wd > 0:
            if mutant == "decay_coupled_l2":
                gs = [g + dtype(wd) * w for g, w in zip(gs, W)]
            else:
                d = dtype(wd * (float(lr_t) if mutant == "decay_with_lr_t" else lr))
                W = [w - w * d for w in W]
        for n in (0, 1):
            g = gs[n]
            if form == "kernel" and not f64:
                M[n] = M[n] + (g - M[n]) * (one - dtype(b1))
                V[n] = V[n] + (g * g - V[n]) * (one - dtype(b2))
            else:
                M[n] = dtype(b1) * M[n] + dtype(1 - b1) * g
                V[n] = dtype(b2) * V[n] + dtype(1 - b2) * (g * g)
        if clip is not None and mutant == "clip_on_m":
            if clip[0] == "clipvalue":
                M = _clip(M, off, clip, None, dtype)
            else:
                M = [m * f for m, f in zip(M, _clip_factors(gs, off, clip, None, dtype))]
        for n in (0, 1):
            W[n] = W[n] - lr_t * M[n] / (np.sqrt(V[n]) + dtype(eps))
            assert W[n].dtype == dtype
        applied += 1
        sched_step += 1
        out.append([w.copy() for w in W])
    return out


def worst(a, b):
    """per net the largest |a - b| over every step"""
    return [max(float(np.abs(x[n] - y[n]).max()) for x, y in zip(a, b)) for n in (0, 1)]


def reference_and_tolerance(case, shape):
    """(inputs, float64 reference per step, tolerance per net): TOL_FACTOR x the worse of the two fp32 mirrors' own error against the
    reference on these very inputs, as adam_reference.tol_adam"""
    inp = case_inputs(case, shape)
    ref = update(case, *inp)
    err = [0.0, 0.0]
    for form in ("kernel", "keras"):
        e = worst(update(case, *inp, dtype=F32, form=form), ref)
        err = [max(a, b) for a, b in zip(err, e)]
    return inp, ref, [TOL_FACTOR * e for e in err]


def pure_decay(case, w0, t0, skip, K):
    """w0 * prod(1 - wd * lr_k) over the applied steps, in float64: what the always-zero class of a gradient schedule follows"""
    c = CASES[case]
    w = np.asarray(w0, dtype=np.float64).copy()
    out, step = [], t0
    for k in range(K):
        if k not in skip:
            w = w * (1.0 - c["wd"] * schedule_lr(c["sched"], step))
            step += 1
        out.append(w.copy())
    return out
