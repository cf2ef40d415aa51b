"""Body of tests/test_gpu_optimizer.py's derived-state tests, shared by two routes: called in-process for the shapes the product
library holds, and run as a script in a fresh child process with KNERF_LIB / KNERF_PROBE_LIB pointing at the `xshape` build variant
(tests/test_gpu_variants.py, keras_nerf_amd/build.py XSHAPES) for the shapes only that library holds: one JSON line per shape.

Everything the forward, dgrad and head kernels read is DERIVED from the fp32 master weights: the bf16 forward stream, the bf16 dgrad
stream, the bias table and the composed head (csrc/knerf_api.hip repack).  Three routes lead there -- knerf_apply_adam (two-net head
launch), knerf_set_weights (one-net launch, null stream) and a device-side write followed by knerf_refresh_weights (the data-parallel
broadcast) -- and from equal masters they must give equal bits in everything that observes the derived state."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

N_POINTS = 8192
ADAM_STEPS = 3
LR = 1e-2          # so that three steps really move the weights (up to 3e-2 each)


def inject(ctx, g_coarse, g_fine):
    """write one gradient per net (REAL layout) into the accumulator [coarse | fine] on the current stream"""
    view = ctx.grads_view()
    n = view.numel() // 2
    for net, g in enumerate((g_coarse, g_fine)):
        half = view[net * n:(net + 1) * n]
        g = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).to(ctx.device)
        if ctx._pad_index is not None:          # width padding: the padded entries keep an exactly zero gradient
            half.zero_()
            half[ctx._pad_index] = g
        else:
            half.copy_(g)


def bits(x: torch.Tensor) -> np.ndarray:
    return x.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def observe(ctx, P, pts, dirs, fused):
    """everything that looks at the derived state, as int32 bit patterns"""
    from keras_nerf_amd.debug import debug_buffer
    from tests.test_gpu_train import flat
    o, d, t, u, img = flat(P)
    out = {}
    for net in (0, 1):
        out[f"query_{net}"] = bits(ctx.query_points(net, pts, dirs))
    r = ctx.render_chunk(o, d, t, u)
    for k in ("c_image", "f_image", "c_weights", "f_weights", "t_fine"):
        out["render_" + k] = bits(r[k])
    ctx.set_option("deterministic", 1)
    ctx.zero_grads()
    loss = torch.zeros(2, device=ctx.device)
    ctx.train_chunk(o, d, t, img, u, inv_chunks=1.0, loss=loss)
    out["train_loss"] = bits(loss)
    out["train_grads"] = bits(ctx.grads_view())
    ctx.zero_grads()
    ctx.set_option("deterministic", 0)
    if fused:
        for net in (0, 1):
            out[f"ext_{net}"] = bits(debug_buffer(ctx, 7, net).view(torch.float32))
    torch.cuda.synchronize()
    for k, v in out.items():
        assert np.isfinite(v.view(np.float32)).all(), k
    return out


def differing(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def check_head(ctx, cfg_run, label):
    """the composed head behind the parameters against float64 of the SAME fp32 masters; (tol_head, worst error) over both nets"""
    from keras_nerf_amd.debug import debug_buffer
    from oracle import nerf_oracle as O
    from tests import adam_reference as A
    Tr, D, rows = A.head_layout(cfg_run)
    worst_tol, worst = 0.0, 0.0
    for net in (0, 1):
        w = ctx.weights_view(net).cpu().numpy()
        if ctx._pad_index is None:
            assert np.array_equal(w.view(np.uint32), ctx.get_weights(net).view(np.uint32))
        else:
            assert np.array_equal(w[ctx._pad_index_host].view(np.uint32), ctx.get_weights(net).view(np.uint32))
        ext = debug_buffer(ctx, 7, net).view(torch.float32).cpu().numpy()
        assert ext.size == w.size + rows * 4 + 4, (label, ext.size, w.size, rows)
        assert np.array_equal(ext[:w.size].view(np.uint32), w.view(np.uint32))
        params = O.unflatten_params(w, cfg_run)
        got = ext[w.size:]
        ref = A.head_fp64(params, cfg_run)
        tol = A.tol_head(params, cfg_run)
        err = float(np.abs(got - ref).max())
        worst_tol, worst = max(worst_tol, tol), max(worst, err)
        assert err <= tol, (label, net, err, tol)
        M = got[:rows * 4].reshape(rows, 4)
        n = cfg_run.n_layers
        assert not M[Tr + D:].view(np.uint32).any(), (label, net, "padding rows")
        assert not M[Tr:, 3].view(np.uint32).any(), (label, net, "sigma column of the direction rows")
        assert np.array_equal(M[:Tr, 3].view(np.uint32), np.ascontiguousarray(params[2 * n][:, 0]).view(np.uint32)), (label, net, "sigma column")
        assert got[rows * 4 + 3:].view(np.uint32)[0] == params[2 * n + 1].view(np.uint32)[0], (label, net, "sigma bias")
    return worst_tol, worst


def run(n_layers=8, dense_units=256, skip_layer=4, pos_emb_xyz=10, pos_emb_dir=4, force_generic=False, expect_fused=True):
    """contexts A (Adam), B (set_weights) and C (device write + refresh_weights) of one shape; raises AssertionError, returns the
    measured head figures"""
    from keras_nerf_amd.runtime import KnerfContext
    from oracle import nerf_oracle as O
    from tests import adam_reference as A
    from tests.problem import make_problem
    label = f"{n_layers}x{dense_units}/{skip_layer} pe {pos_emb_xyz}/{pos_emb_dir}" + (" generic" if force_generic else "")
    cfg = O.NerfConfig(n_layers=n_layers, dense_units=dense_units, skip_layer=skip_layer, pos_emb_xyz=pos_emb_xyz, pos_emb_dir=pos_emb_dir)
    P = make_problem(n_images=1, wh=16, weight_scale=1.5, bias_std=0.05, cfg=cfg)            # 256 rays
    W0 = [O.flatten_params(P["cp"]), O.flatten_params(P["fp"])]
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1.5, 1.5, (N_POINTS, 3)).astype(np.float32)
    dirs = rng.standard_normal((N_POINTS, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    kw = dict(n_layers=n_layers, dense_units=dense_units, skip_layer=skip_layer, pos_emb_xyz=pos_emb_xyz, pos_emb_dir=pos_emb_dir,
              white_background=True, lr=LR, force_generic=force_generic)
    ctxs = []
    res = {"shape": [n_layers, skip_layer, dense_units, pos_emb_xyz, pos_emb_dir], "force_generic": bool(force_generic)}
    try:
        a, b, c = (KnerfContext(**kw) for _ in range(3))
        ctxs = [a, b, c]
        fused = a.get_option("general_shape_path") == 0.0
        assert fused == expect_fused, (label, "general_shape_path", a.get_option("general_shape_path"))
        res["fused"] = fused
        cfg_run = O.NerfConfig(n_layers=n_layers, dense_units=int(a.cfg.dense_units), skip_layer=skip_layer, pos_emb_xyz=pos_emb_xyz,
                               pos_emb_dir=pos_emb_dir)                            # the width the kernels run at (zero-padded)
        n = a.param_count
        assert n == W0[0].size
        for net in (0, 1):
            a.set_weights(net, W0[net]); c.set_weights(net, W0[net])
        at_w0 = observe(c, P, pts, dirs, fused)
        if fused:
            res["head_after_set_weights"] = check_head(c, cfg_run, label + " after set_weights")
        # A: three injected Adam steps (different gradients per net)
        Gc, _ = A.gradient_schedule(n, ADAM_STEPS, 31)
        Gf, _ = A.gradient_schedule(n, ADAM_STEPS, 32)
        for k in range(ADAM_STEPS):
            inject(a, Gc[k], Gf[k])
            a.apply_adam()
        assert a.step == ADAM_STEPS
        WA = [a.get_weights(net) for net in (0, 1)]
        for net in (0, 1):
            moved = np.abs(WA[net] - W0[net])
            assert moved.max() > LR and np.isfinite(WA[net]).all(), (label, net, moved.max())
        # B: the host route to the same masters;  C: the device route (a data-parallel broadcast writes the masters, then refreshes)
        for net in (0, 1):
            b.set_weights(net, WA[net])
            c.weights_view(net).copy_(a.weights_view(net))
        c.refresh_weights()
        oa, ob, oc = (observe(x, P, pts, dirs, fused) for x in (a, b, c))
        assert differing(oa, ob) == [], (label, "apply_adam vs set_weights", differing(oa, ob))
        assert differing(oa, oc) == [], (label, "apply_adam vs refresh_weights", differing(oa, oc))
        # ... and none of the three is still looking at W0
        same = [k for k in oa if np.array_equal(oa[k], at_w0[k])]
        assert same == [], (label, "unchanged by the Adam steps", same)
        if fused:
            res["head_after_adam"] = check_head(a, cfg_run, label + " after apply_adam")
            check_head(c, cfg_run, label + " after refresh_weights")
        # set_weights of one net leaves the other net's derived state alone
        for net in (0, 1):
            b.set_weights(net, W0[net])
            ob2 = observe(b, P, pts, dirs, fused)
            other = 1 - net
            untouched = oa if net == 0 else at_w0       # the other net: still at W_A in the first pass, already back at W0 in the second
            for k in [f"query_{other}"] + ([f"ext_{other}"] if fused else []):
                assert np.array_equal(ob2[k], untouched[k]), (label, "set_weights of net", net, "changed", k)
            assert np.array_equal(ob2[f"query_{net}"], at_w0[f"query_{net}"]), (label, net)
            if net == 1:                                # both nets back at W0: everything as in the beginning
                assert differing(ob2, at_w0) == [], (label, differing(ob2, at_w0))
    finally:
        for x in ctxs:
            x.close()
    return res


def parse(spec):
    v = [int(x) for x in spec.split(",")]
    kw = dict(n_layers=v[0], skip_layer=v[1], dense_units=v[2])
    if len(v) == 5:
        kw.update(pos_emb_xyz=v[3], pos_emb_dir=v[4])
    return kw


if __name__ == "__main__":
    for spec in sys.argv[1:]:
        print(json.dumps(run(**parse(spec))), flush=True)
