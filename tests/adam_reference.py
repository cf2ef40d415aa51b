"""Plain references for the stretch between "a gradient lies in the accumulator" and "the next forward pass runs on new weights"
(csrc/optim.hip adam_kernel / step_status_kernel / head_compose_kernel, csrc/knerf_api.hip knerf_apply_adam): Keras-form Adam in
float64 as oracle.KerasAdam states it, float32 mirrors of it in two operation orders (they MEASURE what fp32 arithmetic alone costs
on a given input; they are not a pass criterion), the gradient schedules the tests inject, ten deliberately wrong Adams, and the
composed head laid out as the extended weight buffer has it (csrc/layout.h).

tests/test_adam_host.py proves on the CPU what the tolerances of tests/test_gpu_optimizer.py rest on, for exactly the cases of the
tables below -- both files take inputs, cases and tolerances from here, so they cannot drift apart."""
import numpy as np

from oracle import nerf_oracle as O

F32 = np.float32

# (lr, beta1, beta2, epsilon) sets that reach the GPU
HYPER = {
    "default": (1e-3, 0.9, 0.999, 1e-7),
    "lr_5e-4": (5e-4, 0.9, 0.999, 1e-7),        # the rate tests/test_gpu_det_skip.py trains with
    "host_logic": (2e-4, 0.8, 0.99, 1e-8),      # tests/test_host_logic.py's pair
}
# case -> (K steps, t0 = applied steps before the first one, indices (from 0) of the poisoned = skipped steps)
CASES = {
    "trajectory": (12, 0, ()),
    "skipped": (12, 0, (4, 9)),
    "queued": (3, 0, (1,)),
    "resume": (6, 30, (2,)),
}
# what the GPU file runs: the trajectory with every hyper-parameter set, the step-count cases with the defaults
GPU_RUNS = [("trajectory", h) for h in HYPER] + [(c, "default") for c in ("skipped", "queued", "resume")]
SEEDS = (11, 12)            # gradient schedules of the coarse / the fine half
W0_SEEDS = (21, 22)         # start weights of the coarse / the fine net
TOL_FACTOR = 8              # on the mirrors' own error: the GPU's double pow / sqrt in lr_t, the hyper-parameters held as float32
POWER_FACTOR = 10           # every mutant must differ from the fp64 reference by more than POWER_FACTOR x the tolerance

# |g| <= G_CAP keeps g * g finite in float32.  A finite |g| > 1.8e19 passes the finite check, makes v = inf and the NEXT step's
# v + (g * g - v) * (1 - b2) NaN (inf - inf).  TensorFlow's own Adam kernel is written in the same form, so the kernel mirrors the
# reference there; the schedules stay below it.
G_CAP = 1e18

ZERO, FIRST_ONLY, CONST_SIGN, FREE = 0, 1, 2, 3


def gradient_schedule(n, K, seed):
    """(list of K float32 gradient vectors [n], class per element).  Per element a magnitude log-uniform in [1e-12, 1e3]; per step
    Gaussian x magnitude with 20 % of the entries exactly 0; classes (5 % each, the rest FREE): ZERO -- always exactly zero;
    FIRST_ONLY -- non-zero at step 1 only (afterwards pure momentum decay: what separates beta1 from beta2); CONST_SIGN."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-12, 3, n)
    c = rng.integers(0, 20, n)
    cls = np.where(c < 3, c, FREE).astype(np.int8)
    G = []
    for k in range(K):
        g = rng.standard_normal(n) * mag
        g[rng.random(n) < 0.2] = 0
        g[cls == ZERO] = 0
        if k > 0:
            g[cls == FIRST_ONLY] = 0
        g[cls == CONST_SIGN] = np.abs(g[cls == CONST_SIGN])
        G.append(np.clip(g, -G_CAP, G_CAP).astype(F32))
    return G, cls


def start_weights(n, seed):
    return np.random.default_rng(seed).normal(0, 0.1, n).astype(F32)


def case_inputs(case, net, n):
    """(w0, gradient list, classes, t0, skip) of one net in one case of CASES: what the GPU test injects and the host test measures"""
    K, t0, skip = CASES[case]
    G, cls = gradient_schedule(n, K, SEEDS[net] + 100 * list(CASES).index(case))
    return start_weights(n, W0_SEEDS[net]), G, cls, t0, skip


def adam_fp64(w0, grads, lr, b1, b2, eps, t0=0, skip=(), mutant=None, every_step=False):
    """Keras-form Adam in float64 (oracle.KerasAdam: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), eps OUTSIDE the root) over the gradient
    vectors `grads`; steps listed in `skip` are omitted entirely (no change of m, v, w or t); the first applied step has t = t0 + 1,
    slots start at zero.  mutant: one deliberate mistake (MUTANTS).  every_step: the list of weights after every step instead."""
    W = np.asarray(w0, dtype=np.float64).copy()
    M, V = np.zeros_like(W), np.zeros_like(W)
    t, left = t0, 0.0
    out = []
    for k, g in enumerate(grads):
        if k in skip:
            if mutant == "skip_advances_t":
                t += 1
            out.append(W.copy())
            continue
        t += 1
        g = np.asarray(g, dtype=np.float64)
        if mutant == "g_not_zeroed":                    # the accumulator keeps what the earlier steps left in it
            g = g + left
            left = g
        tt = {"t_plus_1": t + 1, "t_frozen": 1}.get(mutant, t)
        bb1, bb2, ee = b1, b2, eps
        if mutant == "betas_swapped":
            bb1, bb2 = b2, b1
        if mutant == "beta2_099":
            bb2 = 0.99 if b2 != 0.99 else 0.999
        if mutant == "eps_1e-8":
            ee = 1e-8 if eps != 1e-8 else 1e-7
        lr_t = lr if mutant == "no_bias_correction" else lr * np.sqrt(1 - bb2 ** tt) / (1 - bb1 ** tt)
        M = bb1 * M + (1 - bb1) * g
        V = bb2 * V + (1 - bb2) * g * g
        if mutant == "eps_inside_root":
            W = W - lr_t * M / np.sqrt(V + ee)
        elif mutant == "torch_form":
            W = W - lr * (M / (1 - bb1 ** tt)) / (np.sqrt(V / (1 - bb2 ** tt)) + ee)
        else:
            W = W - lr_t * M / (np.sqrt(V) + ee)
        out.append(W.copy())
    return out if every_step else W


MUTANTS = ("eps_inside_root", "torch_form", "eps_1e-8", "t_plus_1", "t_frozen", "betas_swapped", "beta2_099", "no_bias_correction",
           "skip_advances_t", "g_not_zeroed")


def mutants_for(skip):
    """the mutants that CAN differ on a case: a skipped step that advances t needs a skipped step"""
    return tuple(m for m in MUTANTS if m != "skip_advances_t" or len(skip))


def adam_fp32_mirror(w0, grads, lr, b1, b2, eps, t0=0, skip=(), form="kernel", hyper_f32=False, every_step=False):
    """The same in NumPy float32, one rounding per operation.  form "kernel": m += (g - m)(1 - b1), v += (g g - v)(1 - b2), the order
    of adam_kernel; "keras": b m + (1 - b) g.  lr_t is computed in double and rounded once; hyper_f32: from the float32 values the
    C ABI's knerf_config holds (what step_status_kernel sees) instead of the Python doubles."""
    w = np.asarray(w0, dtype=F32).copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    t = t0
    hl, h1, h2 = (float(F32(x)) for x in (lr, b1, b2)) if hyper_f32 else (lr, b1, b2)
    out = []
    with np.errstate(over="raise"):
        for k, g in enumerate(grads):
            if k in skip:
                out.append(w.copy())
                continue
            t += 1
            g = np.asarray(g, dtype=F32)
            lr_t = F32(hl * np.sqrt(1 - h2 ** t) / (1 - h1 ** t))
            if form == "kernel":
                m = m + (g - m) * (F32(1) - F32(b1))
                v = v + (g * g - v) * (F32(1) - F32(b2))
            elif form == "keras":
                m = F32(b1) * m + F32(1 - b1) * g
                v = F32(b2) * v + F32(1 - b2) * (g * g)
            else:
                raise ValueError(form)
            w = w - lr_t * m / (np.sqrt(v) + F32(eps))
            assert w.dtype == F32 and m.dtype == F32 and v.dtype == F32
            out.append(w.copy())
    return out if every_step else w


def mirror_error(w0, grads, lr, b1, b2, eps, t0=0, skip=(), ref=None):
    """max over both fp32 mirrors and over every step of max |mirror - fp64|: what float32 arithmetic alone costs on these inputs"""
    ref = adam_fp64(w0, grads, lr, b1, b2, eps, t0, skip, every_step=True) if ref is None else ref
    e = 0.0
    for form in ("kernel", "keras"):
        mir = adam_fp32_mirror(w0, grads, lr, b1, b2, eps, t0, skip, form=form, every_step=True)
        e = max(e, max(float(np.abs(a - b).max()) for a, b in zip(mir, ref)))
    return e


def tol_adam(w0, grads, lr, b1, b2, eps, t0=0, skip=(), ref=None):
    return TOL_FACTOR * mirror_error(w0, grads, lr, b1, b2, eps, t0, skip, ref)


# ---- the composed head (csrc/layout.h "collapsed head", csrc/optim.hip head_compose_kernel) ------------------------------------------

def enc_slots(L):
    """slots of a 3 + 6 L wide encoding in the composed head: 16 per k-step, the k-step count even (layout.h enc_q)"""
    return 16 * (((2 + 3 * L + 7) // 8 + 1) // 2 * 2)


def head_layout(cfg):
    """(Tr, D, rows): rows of the trunk output (dense_units, + xyz_dim when the reference concatenates behind the last layer), of the
    direction encoding, and of the head region: dense_units + xyz slots (when concatenated) + dir slots"""
    U = cfg.dense_units
    concat_last = cfg.n_layers > 1 and (cfg.n_layers - 1) % cfg.skip_layer == 0
    Tr = U + (cfg.xyz_dim if concat_last else 0)
    return Tr, cfg.dir_dim, U + (enc_slots(cfg.pos_emb_xyz) if concat_last else 0) + enc_slots(cfg.pos_emb_dir)


def _ext(H, hb, cfg, dtype):
    Tr, D, rows = head_layout(cfg)
    assert H.shape == (Tr + D, 4)
    out = np.zeros(rows * 4 + 4, dtype)
    out[:(Tr + D) * 4] = H.reshape(-1)          # stored by REAL row; the rows up to the slot counts stay zero
    out[rows * 4:] = hb
    return out


def head_fp64(params, cfg):
    """oracle.head_compose on float64 copies of the 24 parameter tensors, as the floats behind the parameters in a net's weight
    buffer: H [rows][4] (columns r, g, b, sigma), then the bias [4]"""
    H, hb = O.head_compose([np.asarray(p, dtype=np.float64) for p in params], cfg)
    return _ext(H, hb, cfg, np.float64)


def head_fp32_mirror(params, cfg):
    """the same products accumulated sequentially in float32 in the loop order of head_compose_kernel (k, then j, ascending; the
    bias from b_c, then b_f, then b_r); measures the fp32 cost, no pass criterion"""
    n, U = cfg.n_layers, cfg.dense_units
    ks, bs, kf, bf, kr, br, kc, bc = (np.asarray(p, dtype=F32) for p in params[2 * n:2 * n + 8])

    def seqmm(a, b):
        out = np.zeros((a.shape[0], b.shape[1]), F32)
        for k in range(a.shape[1]):
            out = out + a[:, k:k + 1] * b[k:k + 1, :]
        return out
    P = seqmm(kr, kc)
    Tr = kf.shape[0]
    H = np.zeros((Tr + kr.shape[0] - U, 4), F32)
    H[:Tr, :3] = seqmm(kf, P[:U])
    H[Tr:, :3] = P[U:]
    H[:Tr, 3] = ks[:, 0]
    hb = bc.copy()
    for j in range(U):
        hb = hb + bf[j] * P[j]
    for k in range(U // 2):
        hb = hb + br[k] * kc[k]
    assert H.dtype == F32 and hb.dtype == F32
    return _ext(H, np.concatenate([hb, bs]), cfg, F32)


def tol_head(params, cfg):
    return TOL_FACTOR * float(np.abs(head_fp32_mirror(params, cfg) - head_fp64(params, cfg)).max())
