"""What tests/test_gpu_objective.py rests on, proved on the CPU (no GPU needed):

* the prefix form of the distortion term and the entropy term of tests/objective_reference.py equal the O(S^2) definition under torch
  float64 autograd (values and gradient with respect to the weights) to 1e-12, on sorted rays of S = 2 ... 257;
* rho and rho' of every loss kind against float64 autograd; keras_nerf_amd.losses' torch forms agree with them;
* for mean squared error without a regulariser the extended reference IS composite_reference.reference, and the extended mirror IS
  composite_reference.mirror32, bit for bit (the extended kernel's plain case is the plain kernel);
* tolerances: tol = 8 x the float32 mirror's error (NumPy's functions; every exp / log / log1p / tanh moved one ulp at random), from
  NumPy alone; the exclusions stay within their cap;
* power: every mutant of objective_reference.MUTANTS is more than 10 x tol away on some output of some case;
* keras_nerf_amd.losses.objective_from: every spelling gives the same record, everything else raises ValueError;
* the ABI refuses a null context / record without touching a device.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import composite_reference as CR
from tests import objective_reference as OR

CHECKED = ("image", "depth", "weights", "draw", "last", "loss") + OR.TERMS
HOST_S = OR.S_CASES
HOST_CASES = [(S, w, n) for S in HOST_S for w in (0, 1) for n in OR.OBJECTIVES]


def test_templates_and_objectives_cover_the_kernel():
    assert sorted({CR.template_C(S) for S in OR.S_CASES}) == [1, 2, 3, 4, 8, 12, 16]
    assert any(S % CR.template_C(S) or S < 64 * CR.template_C(S) for S in OR.S_CASES)
    kinds = {o[0] for o in OR.OBJECTIVES.values()}
    assert kinds == {OR.MSE, OR.MAE, OR.HUBER, OR.LOG_COSH}
    assert any(o[2] and not o[3] for o in OR.OBJECTIVES.values()) and any(o[3] and not o[2] for o in OR.OBJECTIVES.values())
    assert any(o[2] and o[3] and o[0] != OR.MSE for o in OR.OBJECTIVES.values())


def _definition(w, m, delta):
    """D and H of one ray from their definitions, torch float64"""
    D = (w[:, None] * w[None, :] * (m[:, None] - m[None, :]).abs()).sum() + (w * w * delta).sum() / 3.0
    a = w.sum().clamp(float(OR.ACC_LO), float(OR.ACC_HI))
    H = -a * a.log() - (1 - a) * (1 - a).log()
    return D, H


@pytest.mark.parametrize("S", [2, 5, 33, 65, 192, 257])
def test_prefix_form_is_the_definition_under_autograd(S):
    c = CR.case(S, 0)
    sorted_rays = np.flatnonzero(c["cls"] != CR.UNSORTED)
    t = c["t"].astype(np.float64)
    delta = np.concatenate([np.diff(c["t"], axis=1), np.full((len(t), 1), np.float32(1e-10))], axis=1).astype(np.float64)
    w = c["ref"]["weights"]
    m = (t - t[:, :1]) + 0.5 * delta
    D, H, gD, dH = OR.regularizers64(w, m, delta)
    worst = 0.0
    for r in sorted_rays:
        wt = torch.tensor(w[r], dtype=torch.float64, requires_grad=True)
        # the definition uses the absolute midpoints: D is invariant under the shift by t_0
        Dd, Hd = _definition(wt, torch.tensor(t[r] + 0.5 * delta[r]), torch.tensor(delta[r]))
        gDd, = torch.autograd.grad(Dd, wt, retain_graph=True)
        gHd, = torch.autograd.grad(Hd, wt)
        acc = w[r].sum()
        scale = max(1.0, float(np.abs(gDd.numpy()).max()))
        worst = max(worst, abs(D[r] - float(Dd.detach())), abs(H[r] - float(Hd.detach())), float(np.abs(gD[r] - gDd.numpy()).max()) / scale)
        if float(OR.ACC_LO) < acc < float(OR.ACC_HI):
            worst = max(worst, float(np.abs(dH[r] - gHd.numpy()).max()))
        elif acc < float(OR.ACC_LO) or acc > float(OR.ACC_HI):
            assert dH[r] == 0.0 and not gHd.numpy().any()
    print(f"\nS {S}: prefix form vs definition, worst {worst:.2e} over {len(sorted_rays)} sorted rays")
    assert worst < 1e-12


@pytest.mark.parametrize("name,kind,delta", [("mse", OR.MSE, 0.0), ("mae", OR.MAE, 0.0), ("huber", OR.HUBER, 0.25), ("log_cosh", OR.LOG_COSH, 0.0)])
def test_rho_and_its_derivative_against_autograd(name, kind, delta):
    from keras_nerf_amd import losses
    d = torch.tensor(np.concatenate([np.linspace(-1.0, 1.0, 401), [0.0, 0.25, -0.25, 1e-9]]), dtype=torch.float64, requires_grad=True)
    a = d.abs()
    want = {"mse": d * d, "mae": a, "huber": torch.where(a <= delta, 0.5 * d * d, delta * (a - 0.5 * delta)), "log_cosh": torch.log(torch.cosh(d))}[name]
    grad, = torch.autograd.grad(want.sum(), d)
    rho, h = OR.rho64(kind, delta, d.detach().numpy())
    assert np.abs(rho - want.detach().numpy()).max() < 1e-14
    assert np.abs(2.0 * h - grad.numpy()).max() < 1e-14              # sign(0) = 0 is torch's subgradient of |d| at 0 as well
    assert h[401] == 0.0
    spec = losses.loss_from({"huber": {"class_name": "Huber", "config": {"delta": delta}}}.get(name, name))
    y = torch.zeros_like(d)
    assert abs(float(spec(y, d.detach())) - float(want.detach().mean())) < 1e-14


@pytest.mark.parametrize("S,white", [(5, 0), (65, 1), (192, 0), (250, 1)])
def test_plain_objective_is_the_plain_reference_and_mirror_bit_for_bit(S, white):
    c = CR.case(S, white)
    gs, ls = c["grad_scale"], c["loss_scale"]
    ref = OR.reference(c["raw"], c["t"], c["target"], white, gs, ls, 1.0 / CR.R_CASE, OR.PLAIN, own_pixel=c["own"], loss0=CR.LOSS0)
    for k in ("image", "pre", "depth", "weights", "draw"):
        assert np.array_equal(ref[k], c["ref"][k]), k
    assert ref["loss"] == c["ref"]["loss"]
    assert ref["terms"][0] == ref["terms"][1] and abs(ref["terms"][0] - (ref["loss"] - CR.LOSS0)) < 1e-15
    m = OR.mirror32(c["raw"], c["t"], c["target"], white, gs, ls, 1.0 / CR.R_CASE, OR.PLAIN, own_pixel=c["own"])
    p = CR.mirror32(c["raw"], c["t"], c["target"], white, gs, ls, own_pixel=c["own"])
    for k in ("image", "pre", "depth", "weights", "draw", "partial"):
        assert np.array_equal(m[k].view(np.uint32), p[k].view(np.uint32)), k
    assert np.array_equal(m["terms_partial"][0].view(np.uint32), p["partial"].view(np.uint32))


@pytest.mark.parametrize("S,white,name", HOST_CASES)
def test_tolerances_and_exclusions(S, white, name):
    c = OR.case(S, white, name)
    print(f"\nS {S:4d} white {white} {name}: left out {c['n_left_out']} (+ unsorted), acc inside the clamp {c['inside']}; mirror error / tol")
    for k in CHECKED:
        for label in ("numpy", "jitter"):
            assert c["mirror_errs"][label][k] <= c["tol"][k]                    # within tol by construction, both variants
        print(f"    {k:16s} {c['mirror_err'][k]:.2e} / {c['tol'][k]:.2e}")
        assert np.isfinite(c["tol"][k]) and c["tol"][k] > 0
    assert c["n_left_out"] <= 2 and c["inside"] >= 20
    own = c["cls"] == CR.OWN_PIXEL
    assert not c["skip"][own].any()                                              # d == 0 exactly is decided, not left out
    if c["objective"][2] == 0 and c["objective"][3] == 0:
        assert not c["ref"]["draw"][own].any()                                   # sign(0) = 0, clamp(0) = 0, tanh(0) = 0
    else:
        assert not c["ref"]["draw"][own][..., :3].any() and c["ref"]["draw"][own][..., 3].any()
    assert np.isfinite(c["ref"]["draw"]).all()


def _distance(mut, ref, skip, tol):
    e = OR.errors(dict(mut, terms=mut["terms"]), ref, skip)
    return {k: (e[k] / tol[k] if tol[k] > 0 else (np.inf if e[k] > 0 else 0.0)) for k in CHECKED}


def test_every_mutant_is_far_outside_the_tolerances():
    # (objective, nets, net): the fine-only record is what regs_on_wrong_net needs
    runs = [(S, w, n, 3, 0) for S in (5, 192) for w in (0, 1) for n in OR.OBJECTIVES] + [(65, 0, "huber_both", 2, 1), (65, 1, "mse_distortion", 1, 0)]
    best = {m: (0.0, None) for m in OR.MUTANTS}
    for S, white, name, nets, net in runs:
        c = OR.case(S, white, name, nets, net)
        for mutant in OR.MUTANTS:
            mut = OR.reference(c["raw"], c["t"], c["target"], white, c["grad_scale"], c["loss_scale"], c["reg_scale"], c["objective"],
                               net=net, nets=nets, own_pixel=c["own"], loss0=CR.LOSS0, mutant=mutant)
            d = _distance(mut, c["ref"], c["skip"], c["tol"])
            k = max(d, key=d.get)
            if d[k] > best[mutant][0]:
                best[mutant] = (d[k], (S, white, name, k))
    print()
    for mutant, (dist, where) in best.items():
        print(f"    {mutant:32s} {dist:10.3g} x tol at {where}")
    for mutant, (dist, where) in best.items():
        assert dist > CR.POWER_FACTOR, (mutant, dist, where)


def test_objective_from_spellings_and_refusals():
    from keras_nerf_amd import _lib, losses
    rec = lambda *a, **k: losses.record_tuple(losses.objective_from(*a, **k))

    class Huber:                       # what a real tf.keras.losses.Huber looks like from outside
        def __init__(self, delta, reduction="sum_over_batch_size"):
            self.delta, self.reduction = delta, reduction

        def get_config(self):
            return {"name": "huber_loss", "reduction": self.reduction, "delta": self.delta}

        def __call__(self, a, b):
            raise AssertionError("never evaluated")

    class MeanAbsoluteError(Huber):
        def get_config(self):
            return {"name": "mean_absolute_error", "reduction": self.reduction}

    class LogCosh(MeanAbsoluteError):
        pass

    f32 = lambda v: float(np.float32(v))
    assert rec("mse") == rec(None) == rec("mean_squared_error") == rec(losses.MeanSquaredError()) == (0, 0.0, 0.0, 0.0, 3)
    assert losses.is_plain(losses.objective_from("mse")) and losses.is_plain(losses.objective_from("mse", losses.RayRegularizers()))
    mae = (_lib.LOSS_MAE, 0.0, 0.0, 0.0, 3)
    assert rec("mae") == rec("mean_absolute_error") == rec(losses.MeanAbsoluteError()) == rec(MeanAbsoluteError(0)) == \
        rec({"class_name": "MeanAbsoluteError", "config": {"reduction": "sum_over_batch_size"}}) == mae
    hub = (_lib.LOSS_HUBER, f32(0.1), 0.0, 0.0, 3)
    assert rec(losses.Huber(0.1)) == rec(Huber(0.1)) == rec({"class_name": "Huber", "config": {"delta": 0.1}}) == hub
    assert rec("huber") == (_lib.LOSS_HUBER, 1.0, 0.0, 0.0, 3) == rec(losses.Huber()) == rec({"class_name": "Huber", "config": losses.Huber().get_config()})
    lc = (_lib.LOSS_LOG_COSH, 0.0, 0.0, 0.0, 3)
    assert rec("log_cosh") == rec("logcosh") == rec(losses.LogCosh()) == rec(LogCosh(0)) == rec({"class_name": "LogCosh", "config": {}}) == lc
    reg = losses.RayRegularizers(distortion=0.01, opacity_entropy=0.001, nets="fine")
    assert rec("mse", reg) == rec(None, reg.get_config()) == (0, 0.0, f32(0.01), f32(0.001), 2)
    assert not losses.is_plain(losses.objective_from("mse", reg)) and not losses.is_plain(losses.objective_from("mae"))
    assert rec("mae", losses.RayRegularizers(nets="coarse")) == mae                      # no weight set: nets is canonical
    for bad in (lambda a, b: torch.mean(torch.abs(a - b)), "hinge", 3.5, {"class_name": "Hinge", "config": {}},
                {"class_name": "Huber", "config": {"delta": 0.0}}, {"class_name": "Huber", "config": {"delta": -1.0}},
                Huber(0.5, reduction="sum"), {"class_name": "MeanAbsoluteError", "config": {"reduction": "none"}}):
        with pytest.raises(ValueError):
            losses.objective_from(bad)
    with pytest.raises(ValueError, match="sum"):
        losses.objective_from(Huber(0.5, reduction="sum"))
    for kw in (dict(distortion=-0.1), dict(opacity_entropy=-1e-3), dict(distortion=float("nan")), dict(nets="all")):
        with pytest.raises(ValueError):
            losses.RayRegularizers(**kw)
    with pytest.raises(ValueError):
        losses.Huber(delta=0)


def test_compile_refuses_a_loss_before_any_device_work():
    """NeRF.compile validates the objective before it creates a context: the refusals hold on a machine without a GPU"""
    from keras_nerf_amd import losses
    from keras_nerf_amd.model.nerf.nerf import NeRF
    for bad in (lambda a, b: torch.mean(torch.abs(a - b)), "hinge", losses.Huber(0.1).__class__, {"class_name": "Huber", "config": {"delta": -1}}):
        with pytest.raises(ValueError):
            NeRF().compile("adam", bad, batch_size=1, image_height=16, image_width=16, ray_chunks=128)
    with pytest.raises(ValueError):
        NeRF().compile("adam", "mae", batch_size=1, image_height=16, image_width=16, ray_chunks=128, regularizers={"distortion": -1.0})


def test_abi_refuses_null_and_garbage_without_a_device():
    from keras_nerf_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.KnerfObjective) == 20                                          # struct knerf_objective, include/knerf.h
    good = _lib.KnerfObjective(_lib.LOSS_HUBER, 0.5, 0.01, 0.0, 3)
    garbage = _lib.KnerfObjective(77, float("nan"), -1.0, float("inf"), 9)
    out = _lib.KnerfObjective()
    assert lib.knerf_set_objective(None, None, None) == _lib.KNERF_ERR_INVALID
    assert lib.knerf_set_objective(None, None, C.byref(good)) == _lib.KNERF_ERR_INVALID
    assert lib.knerf_set_objective(None, None, C.byref(garbage)) == _lib.KNERF_ERR_INVALID
    assert lib.knerf_get_objective(None, C.byref(out)) == _lib.KNERF_ERR_INVALID
    assert lib.knerf_objective_terms(None, None, None) == _lib.KNERF_ERR_INVALID
