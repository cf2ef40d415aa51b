"""The extended objective of the train step (include/knerf.h knerf_set_objective; csrc/composite_ext.hip): mae / huber / log-cosh
photometric terms, the distortion and the opacity-entropy regulariser -- the kernel on caller-made inputs
(knerf_debug_composite_objective) against the float64 reference of tests/objective_reference.py, then through the context and NeRF.

Cases, ray classes, exclusions and tolerances are tests/objective_reference.py's (tol = 8 x the float32 mirror's error);
tests/test_objective_host.py proves on the CPU what they rest on and that every mutant of the reference is far outside them.  Each
test prints its figures before it asserts (pytest -s).  Measured device error / tol: see tests/README_objective.md.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import composite_reference as CR
from tests import objective_reference as OR
from tests.problem import make_problem
from tests.test_gpu_composite import bits, device_inputs
from tests.test_gpu_composite import train as plain_train

pytestmark = pytest.mark.gpu

_CACHE = {}
SMALL = dict(n_coarse=32, n_fine=64, n_layers=4, dense_units=64, skip_layer=2)      # the smallest fused shape
CHECKED = ("image", "depth", "weights", "draw", "last", "loss")


def record(obj, nets=3):
    from keras_nerf_amd import _lib
    return _lib.KnerfObjective(int(obj[0]), float(obj[1]), float(obj[2]), float(obj[3]), nets)


def ext_train(S, white, obj, **kw):
    """the extended kernel on the case's device inputs (those of tests/test_gpu_composite.py: OWN_PIXEL rays carry the bits of their own
    forward pixel as target)"""
    from keras_nerf_amd import debug
    c, raw, t, target, _ = device_inputs(S, white)
    out = debug.composite_objective(raw, t, target, white, c["grad_scale"], c["loss_scale"], record(obj), 1.0 / CR.R_CASE, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def default_run(S, white, name):
    key = (S, white, name)
    if key not in _CACHE:
        _CACHE[key] = ext_train(S, white, OR.PLAIN if name == "plain" else OR.OBJECTIVES[name], loss0=CR.LOSS0)
    return _CACHE[key]


# ---- 1. values against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OR.OBJECTIVES))
@pytest.mark.parametrize("S,white", [(S, w) for S in OR.S_CASES for w in (0, 1)])
def test_values_against_fp64(S, white, name):
    c = OR.case(S, white, name)
    out, ref, tol, skip = default_run(S, white, name), c["ref"], c["tol"], c["skip"]
    e = CR.errors(dict(out, loss=float(out["loss"][0])), ref, skip)
    for k, tname in enumerate(OR.TERMS):
        e[tname] = abs(float(out["terms"][k]) - float(ref["terms"][k]))
    print(f"\nS {S:4d} white {white} {name}: " + "  ".join(f"{k} {e[k]:.2e}/{tol[k]:.2e}={e[k] / tol[k]:.2f}" for k in e))
    for k in CHECKED + OR.TERMS:
        assert e[k] <= tol[k], (k, e[k], tol[k])
    zero = ~np.abs(ref["draw"]).reshape(len(skip), -1).any(axis=1)
    assert (out["draw"][zero] == 0).all()                          # a ray whose reference draw is all zero is all zero on the device
    own = c["cls"] == CR.OWN_PIXEL
    assert (out["draw"][own][..., :3] == 0).all()                  # d == 0 exactly: sign(0) = clamp(0) = tanh(0) = 0
    if c["objective"][2] == 0 and c["objective"][3] == 0:
        assert zero[np.isin(c["cls"], (CR.RGB_OUTSIDE, CR.OWN_PIXEL))].all()
    assert np.isfinite(out["draw"]).all() and np.isfinite(out["terms"]).all()          # the unsorted class included


# ---- 2. the extended kernel's plain case is the plain kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("S,white", [(S, w) for S in OR.S_CASES + (32,) for w in (0, 1)])
def test_mse_without_regulariser_equals_the_plain_kernel_bit_for_bit(S, white):
    kw = dict(loss0=CR.LOSS0, partial=True)
    if S % 32 == 0:
        kw.update(flags=True)
    a, b = plain_train(S, white, **kw), ext_train(S, white, OR.PLAIN, **kw)
    for k in ("image", "depth", "weights", "draw", "loss", "loss_partial") + (("tile_flags",) if S % 32 == 0 else ()):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(bits(b["terms_partial"][0]), bits(b["terms_partial"][1]))              # rho = d^2: the same operations
    kw = dict(loss0=CR.LOSS0)
    if S % 32 == 0:
        kw.update(tiles=True, count2_start=5, tile_off2=1000)
    a, b = plain_train(S, white, **kw), ext_train(S, white, OR.PLAIN, **kw)
    for k in ("image", "depth", "weights", "draw"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) <= CR.case(S, white)["tol"]["loss"]      # atomics: no fixed order
    if S % 32 == 0:
        n = int(a["tile_count"][0])
        assert n == int(b["tile_count"][0]) and int(a["tile_count2"][0]) == int(b["tile_count2"][0])
        assert np.array_equal(np.sort(a["tile_list"][:n]), np.sort(b["tile_list"][:n]))
        assert np.array_equal(np.sort(a["tile_list2"][5:5 + n]), np.sort(b["tile_list2"][5:5 + n]))
        assert (b["tile_list"][n:] == -1).all() and (b["tile_list2"][5 + n:] == -1).all() and (b["tile_list2"][:5] == -1).all()


# ---- 3. deterministic form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,white,name", [(5, 0, "mae"), (64, 1, "huber_both"), (192, 0, "mse_distortion"), (513, 1, "log_cosh"), (1024, 0, "huber_both")])
def test_loss_and_term_forms(S, white, name):
    c = OR.case(S, white, name)
    obj, ref, tol = c["objective"], c["ref"], c["tol"]
    a = default_run(S, white, name)
    p1, p2 = ext_train(S, white, obj, loss0=CR.LOSS0, partial=True), ext_train(S, white, obj, loss0=CR.LOSS0, partial=True)
    for k in ("loss", "loss_partial", "terms", "terms_partial"):
        assert np.array_equal(bits(p1[k]), bits(p2[k])), k
    print(f"\nS {S} white {white} {name}: loss atomic {a['loss'][0]!r} partial {p1['loss'][0]!r} fp64 {ref['loss']!r} tol {tol['loss']:.2e}")
    for out in (a, p1):
        assert abs(float(out["loss"][0]) - ref["loss"]) <= tol["loss"]
        for k, tname in enumerate(OR.TERMS):
            assert abs(float(out["terms"][k]) - ref["terms"][k]) <= tol[tname], tname
    assert p1["loss_partial"].shape == ref["partial"].shape and np.abs(p1["loss_partial"] - ref["partial"]).sum() <= tol["loss"]
    for k, tname in enumerate(OR.TERMS):
        assert np.abs(p1["terms_partial"][k] - ref["terms_partial"][k]).sum() <= tol[tname], tname
    for k in ("image", "draw", "weights"):
        assert np.array_equal(bits(p1[k]), bits(a[k]))


# ---- 4. tile flags and lists ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", OR.TILE_S)
@pytest.mark.parametrize("name", ["mae", "mse_distortion"])
def test_tile_flags_and_lists_follow_the_final_draw(S, name):
    white = 1
    c = OR.case(S, white, name)
    obj = c["objective"]
    R, nt = CR.R_CASE, S // 32
    f = ext_train(S, white, obj, loss0=CR.LOSS0, flags=True, partial=True)
    l = ext_train(S, white, obj, loss0=CR.LOSS0, tiles=True, count2_start=37, tile_off2=100_000)
    assert np.array_equal(bits(f["draw"]), bits(l["draw"]))
    want = CR.dead_tiles(f["draw"], c["raw"])                      # composite.hip's dead rule on the device's own draw and raw
    assert np.array_equal(f["tile_flags"], want)
    live = np.flatnonzero(want).astype(np.int32)
    n = int(l["tile_count"][0])
    print(f"\nS {S} {name}: {n} of {R * nt} tiles live")
    assert n == len(live) and 0 < n < R * nt
    assert np.array_equal(np.sort(l["tile_list"][:n]), live) and (l["tile_list"][n:] == -1).all()
    assert int(l["tile_count2"][0]) == 37 + n and np.array_equal(np.sort(l["tile_list2"][37:37 + n]), live + 100_000)
    per_ray = want.reshape(R, nt)
    own = c["cls"] == CR.OWN_PIXEL
    assert (f["draw"][own][..., :3] == 0).all()                    # no photometric gradient on a ray that hits its target
    if obj[2]:
        assert per_ray[own].any(axis=1).all() and (f["draw"][own][..., 3] != 0).any(axis=1).all()      # ... but the regulariser's
    else:
        assert not per_ray[own].any()


# ---- 5. end to end, exact: Huber(2) never saturates on |d| <= 1, its step is half the mse step ------------------------------------------
def _small_problem():
    if "P" not in _CACHE:
        _CACHE["P"] = make_problem(n_images=1, wh=16, weight_scale=1.5, bias_std=0.05, cfg=O.NerfConfig(**SMALL))
    return _CACHE["P"]


def _flat(P):
    N = P["N"]
    return P["o"].reshape(N, 3), P["d"].reshape(N, 3), P["t"].reshape(N, -1), P["u"].reshape(N, -1), P["img"].reshape(N, 3)


def _ctx(P, **kw):
    from keras_nerf_amd.runtime import KnerfContext
    opts = dict(kw.pop("options", {}))
    ctx = KnerfContext(white_background=True, options=opts, **SMALL, **kw)
    ctx.set_weights(0, O.flatten_params(P["cp"]))
    ctx.set_weights(1, O.flatten_params(P["fp"]))
    return ctx


def _occupancy(ctx):
    rng = np.random.default_rng(3)
    for net in (0, 1):
        ctx.set_occupancy(net, rng.random((8, 8, 8)) < 0.6, (-1.5,) * 3, (1.5,) * 3, "occupied")
    ctx.set_option("occupancy_train", 1)


@pytest.mark.parametrize("general", [False, True], ids=["fused", "general"])
@pytest.mark.parametrize("occupancy", [False, True], ids=["dense", "occupancy"])
def test_huber_that_never_saturates_is_half_the_mse_step_exactly(general, occupancy):
    from keras_nerf_amd import losses
    P = _small_problem()
    o, d, t, u, img = _flat(P)
    ctx = _ctx(P, options={"deterministic": 1}, force_generic=general)
    if occupancy:
        _occupancy(ctx)
    got = {}
    for name, loss in (("mse", "mse"), ("huber", losses.Huber(delta=2.0))):
        if name != "mse":
            ctx.set_objective(loss=loss)
        acc = torch.zeros(2, device="cuda")
        ctx.train_batch(o, d, t, img, u, ray_chunks=128, loss=acc)          # two chunks of 128 rays, merged into one launch
        torch.cuda.synchronize()
        got[name] = (ctx.grads_view().cpu().numpy().copy(), acc.cpu().numpy(), ctx.objective_terms().cpu().numpy())
        ctx.zero_grads()
    ctx.close()
    g, h = got["mse"][0], got["huber"][0]
    big = np.abs(g) >= 1e-30
    assert big.sum() > 0.5 * g.size and np.isfinite(h).all()
    assert np.array_equal(bits(g[big]), bits((h * np.float32(2.0))[big]))
    for net in (0, 1):
        lm, lh = got["mse"][1][net], got["huber"][1][net]
        assert abs(float(lh) - 0.5 * float(lm)) <= float(np.spacing(np.float32(0.5 * lm))), (net, lm, lh)
    assert not got["mse"][2].any()                                       # the plain kernel computes no terms
    tm = got["huber"][2]
    assert np.array_equal(bits(tm[:, 0]), bits(got["huber"][1])) and (tm[:, 1] > 0).all()         # photometric = the loss; the mse beside it
    assert np.allclose(tm[:, 1], got["mse"][1], rtol=1e-6)


# ---- 6. end to end, against the oracle's arithmetic -----------------------------------------------------------------------------------
def test_mae_with_both_regularisers_against_the_oracle():
    from keras_nerf_amd import losses
    from keras_nerf_amd.debug import debug_buffer
    from tests.test_gpu_train import per_tensor_err
    from tests.test_gpu_wgrad_regime import GRAD_TOL_EMU
    P = _small_problem()
    cfg = P["cfg"]
    R, Na = 128, cfg.n_coarse + cfg.n_fine
    o, d, t, u, img = (x[:R] for x in _flat(P))
    obj = (OR.MAE, 0.0, 0.01, 0.001)
    ctx = _ctx(P)
    ctx.set_objective(loss="mae", regularizers=losses.RayRegularizers(distortion=0.01, opacity_entropy=0.001))
    loss = torch.zeros(2, device="cuda")
    ctx.train_batch(o, d, t, img, u, ray_chunks=R, loss=loss)
    torch.cuda.synchronize()
    g, n = ctx.grads_view().cpu().numpy(), ctx.param_count
    terms = ctx.objective_terms().cpu().numpy().astype(np.float64)
    t_fine = debug_buffer(ctx, 5).view(torch.float32).cpu().numpy()[:R * Na].reshape(R, Na)
    raw_fine = debug_buffer(ctx, 3).view(torch.float32).cpu().numpy()[:R * Na * 4].reshape(R, Na, 4).copy()
    loss = loss.cpu().numpy()
    ctx.close()
    gs, ls, rs = 2.0 / (3.0 * R), 1.0 / (3.0 * R), 1.0 / R
    for net, (params, tt) in enumerate(((P["cp"], t), (P["fp"], t_fine))):
        res, (mc, _) = O.predict_and_render_chunk_single(params, o, d, tt, cfg, True, emulate_bf16=O.FUSED, want_cache=True)
        raw = np.concatenate([res["rgb"], res["sigma"].reshape(R, -1, 1)], axis=-1).astype(np.float32)
        ref = OR.reference(raw, np.ascontiguousarray(tt, np.float32), img, 1, gs, ls, rs, obj)
        grads = O.mlp_backward(params, mc, ref["draw"][..., :3].astype(np.float32), ref["draw"][..., 3].astype(np.float32), cfg)
        e = per_tensor_err(g[net * n:(net + 1) * n], O.flatten_params(grads), cfg)
        print(f"\nnet {net}: worst per-tensor gradient error {e[0]:.2e} ({e[1]}), bound {GRAD_TOL_EMU}; loss {loss[net]:.6f} oracle {ref['loss']:.6f}")
        assert e[0] < GRAD_TOL_EMU, e
        # the oracle's forward differs from the device's by the bf16 arithmetic's noise: the project's bound for losses compared that way
        # (the terms are held to their own tolerance below, on the raw the device itself produced)
        assert abs(float(loss[net]) - ref["loss"]) < 2e-3
    # the fine pass's terms on the device's OWN raw and t (what the compositing kernel read), at the tolerance of its own mirror
    ref = OR.reference(raw_fine, t_fine, img, 1, gs, ls, rs, obj)
    tol = {}
    for fn in (OR.math_numpy(), OR.math_jittered(11)):
        m = OR.mirror32(raw_fine, t_fine, img, 1, gs, ls, rs, obj, fn=fn)
        for k, name in enumerate(OR.TERMS):
            tol[name] = max(tol.get(name, 0.0), CR.TOL_FACTOR * CR.loss_mirror_error(m["terms_partial"][k], ref["terms_partial"][k], 0.0))
        tol["loss"] = max(tol.get("loss", 0.0), CR.TOL_FACTOR * CR.loss_mirror_error(m["partial"], ref["partial"], 0.0))
    for k, name in enumerate(OR.TERMS):
        print(f"fine {name}: device {terms[1][k]:.8f} fp64 {ref['terms'][k]:.8f} tol {tol[name]:.2e}")
        assert abs(terms[1][k] - ref["terms"][k]) <= tol[name], name
    assert abs(float(loss[1]) - ref["loss"]) <= tol["loss"]


# ---- 7. public interface --------------------------------------------------------------------------------------------------------------
def _nerf(P, loss="mse", regularizers=None, **kw):
    from keras_nerf_amd.model.nerf.nerf import NeRF
    m = NeRF(pos_emb_xyz=10, pos_emb_dir=4, **SMALL)
    m.compile("adam", loss, batch_size=1, image_height=16, image_width=16, ray_chunks=128, white_background=True, regularizers=regularizers, **kw)
    m.coarse.set_flat_weights(O.flatten_params(P["cp"])); m.fine.set_flat_weights(O.flatten_params(P["fp"]))
    return m


def test_compile_accepts_the_objective_in_every_spelling():
    from keras_nerf_amd import _lib, losses
    P = _small_problem()
    batch = (P["img"], (P["o"], P["d"], P["t"]))
    want = {"mae": (_lib.LOSS_MAE, 0.0, 0.0, 0.0, 3), "huber": (_lib.LOSS_HUBER, float(np.float32(0.1)), float(np.float32(0.01)), 0.0, 3)}
    runs = (("mae", "mae", None), ("huber", losses.Huber(0.1), losses.RayRegularizers(distortion=0.01)),
            ("huber", {"class_name": "Huber", "config": {"delta": 0.1, "reduction": "sum_over_batch_size"}}, {"distortion": 0.01}))
    for key, loss, reg in runs:
        m = _nerf(P, loss, reg)
        assert losses.record_tuple(m._ctx.get_objective()) == want[key]
        w0 = m.coarse.get_flat_weights().copy()
        logs = m.train_step(batch, u=P["u"])                        # sync: a non-finite gradient would raise from here
        terms = m.objective_terms()
        assert np.isfinite(float(logs["coarse_loss"])) and np.isfinite(float(logs["fine_loss"]))
        w1 = m.coarse.get_flat_weights()
        assert np.isfinite(w1).all() and 0 < np.abs(w1 - w0).max() < 1e-2
        for name in ("coarse", "fine"):
            tt = terms[name]
            assert set(tt) == {"photometric", "mse", "distortion", "opacity_entropy", "total"}
            assert abs(tt["total"] - float(logs[name + "_loss"])) <= 1e-6 * max(1.0, tt["total"])
            assert tt["mse"] > 0 and tt["distortion"] > 0 and tt["opacity_entropy"] > 0
        assert m.metrics_names == ["coarse_loss", "coarse_psnr", "coarse_ssim", "fine_loss", "fine_psnr", "fine_ssim"]


def test_ray_mode_psnr_comes_from_the_squared_error_and_test_step_reports_the_chosen_loss():
    P = _small_problem()
    o, d, t, u, img = _flat(P)
    m = _nerf(P, "mae")
    logs = m.train_step((img, (o, d, t)), u=P["u"])                # a 2-D target: a batch of scattered rays
    terms = m.objective_terms()
    for name in ("coarse", "fine"):
        assert abs(float(logs[name + "_psnr"]) - (-10.0 * np.log10(terms[name]["mse"]))) < 1e-4
        assert abs(float(logs[name + "_psnr"]) - (-10.0 * np.log10(terms[name]["photometric"]))) > 0.1        # not the MAE's
        assert abs(float(logs[name + "_loss"]) - terms[name]["photometric"]) < 1e-6
    m.reset_metrics()
    rays = (P["o"], P["d"], P["t"])
    logs = m.test_step((P["img"], rays), u=P["u"])
    coarse, fine = m.predict_and_render_images(rays, u=P["u"], outputs=("image",))
    target = torch.as_tensor(P["img"], device="cuda")
    for name, out in (("coarse", coarse), ("fine", fine)):
        want = float(torch.mean(torch.abs(out["image"] - target)))
        assert abs(float(logs[name + "_loss"]) - want) < 1e-6, (name, float(logs[name + "_loss"]), want)
        assert abs(float(logs[name + "_psnr"]) - float(-10.0 * torch.log10(torch.mean((out["image"] - target) ** 2)))) < 1e-3


def test_mse_after_another_objective_is_plain_again():
    from keras_nerf_amd import losses
    P = _small_problem()
    batch = (P["img"], (P["o"], P["d"], P["t"]))
    a = _nerf(P, "log_cosh", losses.RayRegularizers(opacity_entropy=0.001), deterministic=True)
    a.train_step(batch, u=P["u"])
    a.compile("adam", "mse", batch_size=1, image_height=16, image_width=16, ray_chunks=128, white_background=True, deterministic=True)
    a.coarse.set_flat_weights(O.flatten_params(P["cp"])); a.fine.set_flat_weights(O.flatten_params(P["fp"]))
    b = _nerf(P, "mse", deterministic=True)
    assert losses.is_plain(a._ctx.get_objective()) and losses.record_tuple(a._ctx.get_objective()) == losses.record_tuple(b._ctx.get_objective())
    la, lb = a.train_step(batch, u=P["u"]), b.train_step(batch, u=P["u"])
    for net in ("coarse", "fine"):
        assert np.array_equal(bits(getattr(a, net).get_flat_weights()), bits(getattr(b, net).get_flat_weights()))
        assert float(la[net + "_loss"]) == float(lb[net + "_loss"])
    assert not any(a.objective_terms()["fine"].values())


# ---- 8. it does something -------------------------------------------------------------------------------------------------------------
def test_distortion_penalty_lowers_the_distortion():
    from keras_nerf_amd import losses
    from keras_nerf_amd.model.nerf.nerf import NeRF
    from tests.procedural_scene import make_scene
    shape = dict(n_coarse=64, n_fine=64, n_layers=4, dense_units=64, skip_layer=2)
    measure = losses.objective_from("mse", losses.RayRegularizers(distortion=0.01))
    final = {}
    for lam in (0.01, 0.0):
        m = NeRF(seed=5, **shape)
        m.compile("adam", "mse", batch_size=1, image_height=16, image_width=16, ray_chunks=256, white_background=True, deterministic=True,
                  regularizers=losses.RayRegularizers(distortion=lam))
        if "scene" not in _CACHE:
            _CACHE["scene"] = make_scene(m._ctx, wh=16, n_views=1)
        o, d, t, img = _CACHE["scene"]
        u = torch.as_tensor(np.random.default_rng(9).random((1, 16, 16, 64), dtype=np.float32), device="cuda")
        for _ in range(60):
            m.train_step((img, (o, d, t)), u=u, with_metrics=False, sync=False)
        # both runs measured the same way: one more pass under the penalising objective, whose terms are read (no optimizer step)
        m._ctx.set_objective(measure)
        m._ctx.train_batch(o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1, 64), img.reshape(-1, 3), u.reshape(-1, 64), ray_chunks=256)
        final[lam] = m.objective_terms()["fine"]["distortion"]
        m._ctx.poll_nonfinite(wait=True)
    print(f"\nfine distortion after 60 steps: penalised {final[0.01]:.6f}, not penalised {final[0.0]:.6f}")
    assert np.isfinite(final[0.01]) and final[0.01] < final[0.0]
