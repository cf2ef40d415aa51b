"""GPU parity of the training path (knerf_train_chunk / knerf_apply_adam) against the CPU oracle.

Gradients: compared per tensor against the oracle in the kernels' arithmetic (emulate_bf16: bf16 matmul operands, fp32
accumulate) to 2.5e-2 of the tensor's max |g|, and against the fp32 oracle (the reference's arithmetic) to 8e-2 (about
twice the measured 1.1e-2 / 5e-2); the measured values are logged.  Adam: weights after several steps with the training kernels' own
gradients against the oracle's Keras-form Adam -- loosely (direction and 3 % of the movement: the gradients carry 1 % bf16 noise); the
exact comparison of the update, the step count and the re-packing, with injected gradients against float64, is tests/test_gpu_optimizer.py."""
import numpy as np
import pytest
from keras_nerf_amd.debug import debug_buffer
import torch

from oracle import nerf_oracle as O
from tests.problem import make_problem
from tests.test_gpu_forward import log_stats

pytestmark = pytest.mark.gpu


def new_ctx(P, **kw):
    from keras_nerf_amd.runtime import KnerfContext
    ctx = KnerfContext(white_background=True, **kw)
    ctx.set_weights(0, O.flatten_params(P["cp"]))
    ctx.set_weights(1, O.flatten_params(P["fp"]))
    return ctx


def flat(P):
    N = P["N"]
    return P["o"].reshape(N, 3), P["d"].reshape(N, 3), P["t"].reshape(N, -1), P["u"].reshape(N, -1), P["img"].reshape(N, 3)


def per_tensor_err(g, ref, cfg):
    off, worst = 0, (0.0, "")
    for name, fi, fo in O.layer_shapes(cfg):
        for kind, n in (("kernel", fi * fo), ("bias", fo)):
            a, b = g[off:off + n], ref[off:off + n]
            e = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))
            if e > worst[0]:
                worst = (e, f"{name}/{kind}")
            off += n
    return worst


def test_train_chunk_gradients_and_losses():
    P = make_problem(n_images=1, wh=16, weight_scale=1.5, bias_std=0.05)
    cfg = P["cfg"]
    ctx = new_ctx(P)
    o, d, t, u, img = flat(P)
    loss = torch.zeros(2, device="cuda")
    ci = torch.empty((P["N"], 3), device="cuda"); fi = torch.empty_like(ci)
    ctx.train_chunk(o, d, t, img, u, inv_chunks=1.0, loss=loss, c_image=ci, f_image=fi)
    torch.cuda.synchronize()
    g = ctx.grads_view().cpu().numpy()
    n = ctx.param_count
    t_fine = debug_buffer(ctx, 5).view(torch.float32).cpu().numpy()[:P["N"] * 192].reshape(P["N"], 192)
    import os
    from tests.test_gpu_forward import OUT
    os.makedirs(OUT, exist_ok=True)
    _rc, _lc, _gc = O.chunk_loss_and_grads(P["cp"], o, d, t, img, cfg, True, emulate_bf16=O.FUSED)
    _rf, _lf, _gf = O.chunk_loss_and_grads(P["fp"], o, d, t_fine, img, cfg, True, emulate_bf16=O.FUSED)
    np.savez(os.path.join(OUT, "train_debug.npz"), g=g, gc=O.flatten_params(_gc), gf=O.flatten_params(_gf),
             draw=debug_buffer(ctx, 4).view(torch.float32).cpu().numpy()[:P["N"] * 192 * 4],
             act=debug_buffer(ctx, 0).cpu().numpy()[:2 * 118 * 1024], mask=debug_buffer(ctx, 1).cpu().numpy()[:2 * 8 * 1024],
             dz=debug_buffer(ctx, 2).cpu().numpy()[:2 * 130 * 1024],
             raw=debug_buffer(ctx, 3).view(torch.float32).cpu().numpy()[:P["N"] * 192 * 4], t_fine=t_fine)
    for emu, tol in ((O.FUSED, 2.5e-2), (False, 8e-2)):
        rc, lc, gc = O.chunk_loss_and_grads(P["cp"], o, d, t, img, cfg, True, emulate_bf16=emu)
        rf, lf, gf = O.chunk_loss_and_grads(P["fp"], o, d, t_fine, img, cfg, True, emulate_bf16=emu)
        ec = per_tensor_err(g[:n], O.flatten_params(gc), cfg)
        ef = per_tensor_err(g[n:], O.flatten_params(gf), cfg)
        log_stats(f"train_chunk_grads_emulate_{emu}", coarse_worst=ec[0], fine_worst=ef[0],
                  loss_c=abs(float(loss[0]) - float(lc)), loss_f=abs(float(loss[1]) - float(lf)))
        assert ec[0] < tol, ec
        assert ef[0] < tol, ef
        assert abs(float(loss[0]) - float(lc)) < 2e-3 and abs(float(loss[1]) - float(lf)) < 2e-3
        if emu:
            np.testing.assert_allclose(ci.cpu().numpy(), rc["image"], atol=1e-2)
            np.testing.assert_allclose(fi.cpu().numpy(), rf["image"], atol=1e-2)
    assert np.abs(g[:n]).max() > 1e-6 and np.abs(g[n:]).max() > 1e-6
    ctx.close()


def test_gradient_accumulation_over_chunks_and_zeroing():
    P = make_problem(n_images=1, wh=16, weight_scale=1.5, bias_std=0.05)
    ctx = new_ctx(P)
    o, d, t, u, img = flat(P)
    ctx.train_chunk(o, d, t, img, u, inv_chunks=1.0)
    g_full = ctx.grads_view().clone()
    ctx.zero_grads()
    assert float(ctx.grads_view().abs().max()) == 0.0
    # two half chunks with inv_chunks = 1/2 accumulate to the full-batch gradient (nerf.py:383-384)
    h = P["N"] // 2
    for i in range(2):
        sl = slice(i * h, (i + 1) * h)
        ctx.train_chunk(o[sl], d[sl], t[sl], img[sl], u[sl], inv_chunks=0.5, ray_offset=i * h)
    g_acc = ctx.grads_view()
    rel = float((g_acc - g_full).abs().max() / g_full.abs().max())
    log_stats("grad_accumulation", rel=rel)
    assert rel < 2e-3       # fp32 atomics: order differs, values agree
    ctx.close()


def test_adam_steps_follow_oracle():
    # glorot-scale weights: the x1.5 problem reacts chaotically to a 1e-3 Adam step (loss 0.19 -> 0.32), which would
    # turn this into a test of rounding noise
    P = make_problem(n_images=1, wh=16, weight_scale=1.0, bias_std=0.0)
    cfg = P["cfg"]
    ctx = new_ctx(P)
    o, d, t, u, img = flat(P)
    cp = [p.copy() for p in P["cp"]]; fp = [p.copy() for p in P["fp"]]
    oc, of_ = O.KerasAdam(cp), O.KerasAdam(fp)
    R = 128
    loss = torch.zeros(2, device="cuda")
    for step in range(3):
        loss.zero_()
        for c in range(P["N"] // R):
            sl = slice(c * R, (c + 1) * R)
            ctx.train_chunk(o[sl], d[sl], t[sl], img[sl], u[sl], inv_chunks=R / P["N"], loss=loss, ray_offset=c * R)
        ctx.apply_adam()
        m, _, _, _ = O.train_step(cp, fp, oc, of_, P["img"], P["o"], P["d"], P["t"], P["u"], cfg, R, True, "zero",
                                  emulate_bf16=O.FUSED)
        lg = loss.cpu().numpy()
        log_stats(f"adam_step_{step}", loss_c_gpu=lg[0], loss_c_ref=m["coarse_loss"], loss_f_gpu=lg[1], loss_f_ref=m["fine_loss"])
        assert abs(lg[0] - m["coarse_loss"]) < 3e-3 and abs(lg[1] - m["fine_loss"]) < 3e-3
    assert ctx.step == 3
    wc = ctx.get_weights(0); wf = ctx.get_weights(1)
    for w, ref, init in ((wc, O.flatten_params(cp), O.flatten_params(P["cp"])), (wf, O.flatten_params(fp), O.flatten_params(P["fp"]))):
        moved = np.abs(ref - init) > 1e-4
        agree = np.mean(np.sign(w - init)[moved] == np.sign(ref - init)[moved])
        log_stats("adam_direction_agreement", agree=agree, mean_abs_diff=np.abs(w - ref).mean(), mean_abs_move=np.abs(ref - init).mean())
        assert agree > 0.995                                            # measured 0.9984 / 0.9999
        assert np.abs(w - ref).mean() < 0.03 * np.abs(ref - init).mean()   # measured 0.2 % / 1.1 % of the movement
    # gradients were zeroed by apply_adam (nerf.py:464-471)
    assert float(ctx.grads_view().abs().max()) == 0.0
    ctx.close()


def test_nonfinite_gradient_raises_and_leaves_weights_untouched():
    from keras_nerf_amd.runtime import NonFiniteGradientError
    P = make_problem(n_images=1, wh=16)
    ctx = new_ctx(P)
    before = ctx.get_weights(0)
    ctx.grads_view()[123] = float("nan")
    with pytest.raises(NonFiniteGradientError):
        ctx.apply_adam()
    np.testing.assert_array_equal(ctx.get_weights(0), before)
    assert ctx.step == 0
    # the skipped step cleared the accumulators (a caller that catches the error and goes on must not add onto NaN) ...
    assert float(ctx.grads_view().abs().max()) == 0.0
    # ... and the context keeps working: a good step after the bad one is applied as step 1
    o, d, t, u, img = flat(P)
    ctx.train_chunk(o, d, t, img, u)
    ctx.apply_adam()
    assert ctx.step == 1 and np.abs(ctx.get_weights(0) - before).max() > 0
    # asynchronous form: nothing raises at apply time, the poll reports it once, later polls are clean
    ctx.grads_view()[7] = float("inf")
    w1 = ctx.get_weights(1)
    ctx.apply_adam(check=False)
    with pytest.raises(NonFiniteGradientError):
        ctx.poll_nonfinite(wait=True)
    ctx.poll_nonfinite(wait=True)
    assert ctx.step == 1
    np.testing.assert_array_equal(ctx.get_weights(1), w1)
    ctx.close()


def test_ragged_chunk_training_matches_oracle():
    # 37 rays: n_rays*S is not a multiple of the 256-sample workgroup nor of the 32-sample tile; padded lanes must
    # contribute nothing to the gradients
    P = make_problem(n_images=1, wh=16, weight_scale=1.5, bias_std=0.05)
    cfg = P["cfg"]
    ctx = new_ctx(P)
    o, d, t, u, img = [x[:37].copy() for x in flat(P)]
    big = flat(P)
    ctx.train_chunk(big[0], big[1], big[2], big[4], big[3])      # leave stale data of a larger chunk in the workspaces
    ctx.zero_grads()
    loss = torch.zeros(2, device="cuda")
    ctx.train_chunk(o, d, t, img, u, loss=loss)
    g = ctx.grads_view().cpu().numpy()
    n = ctx.param_count
    rc, lc, gc = O.chunk_loss_and_grads(P["cp"], o, d, t, img, cfg, True, emulate_bf16=O.FUSED)
    ec = per_tensor_err(g[:n], O.flatten_params(gc), cfg)
    log_stats("ragged_train_chunk", coarse_worst=ec[0], loss_c=abs(float(loss[0]) - float(lc)))
    assert ec[0] < 2.5e-2, ec
    assert abs(float(loss[0]) - float(lc)) < 2e-3
    ctx.close()


@pytest.mark.parametrize("n_coarse,n_fine,white,oob", [(32, 64, False, "zero"), (48, 80, True, "clamp"), (64, 0, False, "zero"),
                                                       (256, 256, True, "zero"),      # the largest counts the kernels accept
                                                       (2, 3, False, "clamp")])       # and the smallest
def test_other_sample_counts_backgrounds_and_oob(n_coarse, n_fine, white, oob):
    """sample counts other than 64+128 (the reference's own tests use 32), black background, clamp mode, and n_fine = 0"""
    from keras_nerf_amd.runtime import KnerfContext
    cfg = O.NerfConfig(n_coarse=n_coarse, n_fine=n_fine)
    P = make_problem(n_images=1, wh=4 if n_coarse == 256 else 8, weight_scale=1.5, bias_std=0.05, cfg=cfg)
    N = P["N"]
    o, d, t, img = P["o"].reshape(N, 3), P["d"].reshape(N, 3), P["t"].reshape(N, -1), P["img"].reshape(N, 3)
    u = P["u"].reshape(N, -1) if n_fine else None
    ctx = KnerfContext(n_coarse=n_coarse, n_fine=n_fine, white_background=white, oob=oob)
    ctx.set_weights(0, O.flatten_params(P["cp"])); ctx.set_weights(1, O.flatten_params(P["fp"]))
    ci, cd, cw = [x.cpu().numpy() for x in ctx.forward_chunk(0, o, d, t)]
    rc = O.predict_and_render_chunk_single(P["cp"], o, d, t, cfg, white, emulate_bf16=O.FUSED)
    np.testing.assert_allclose(ci, rc["image"], atol=1e-2); np.testing.assert_allclose(cw, rc["weights"], atol=1e-2)
    if n_fine == 0:               # coarse-only TRAINING is covered by tests/test_gpu_configs.py
        ctx.close(); return
    loss = torch.zeros(2, device="cuda")
    ctx.train_chunk(o, d, t, img, u, loss=loss)
    g = ctx.grads_view().cpu().numpy(); n = ctx.param_count
    t_fine = debug_buffer(ctx, 5).view(torch.float32).cpu().numpy()[:N * (n_coarse + n_fine)].reshape(N, n_coarse + n_fine)
    np.testing.assert_array_equal(t_fine, O.fine_points(t, debug_buffer(ctx, 6).view(torch.float32).cpu().numpy()[:N * n_coarse].reshape(N, n_coarse), u, oob))
    _, lc, gc = O.chunk_loss_and_grads(P["cp"], o, d, t, img, cfg, white, emulate_bf16=O.FUSED)
    _, lf, gf = O.chunk_loss_and_grads(P["fp"], o, d, t_fine, img, cfg, white, emulate_bf16=O.FUSED)
    ec, ef = per_tensor_err(g[:n], O.flatten_params(gc), cfg), per_tensor_err(g[n:], O.flatten_params(gf), cfg)
    log_stats(f"config_{n_coarse}_{n_fine}_{white}_{oob}", coarse_worst=ec[0], fine_worst=ef[0])
    tol = 8e-2 if n_coarse == 2 else 2.5e-2     # 128 + 320 samples in all: the bf16 roundings do not average out (measured 5.4e-2)
    assert ec[0] < tol and ef[0] < tol, (ec, ef)
    assert abs(float(loss[0]) - float(lc)) < 2e-3 and abs(float(loss[1]) - float(lf)) < 2e-3
    ctx.close()
