"""What the tolerances of tests/test_gpu_composite.py rest on, proved on the CPU (no GPU needed) for exactly the cases that file uses
(tests/composite_reference.py CASES: 97 rays, 18 sample counts, both backgrounds, ten ray classes):

* tie to the oracle: reference() fed float64 inputs equals oracle.render_image_depth_chunk + oracle.render_backward in float64, the
  pair tests/test_oracle_grad.py checks against autograd;
* tolerance: tol = 8 x the error of the float32 mirror of the kernel against reference(), the larger of two mirrors (NumPy's exp;
  exp with every result moved one ulp at random), per output and per case, computed at run time from NumPy alone, never from GPU
  output.  The loss is one number, so its figure is the bound of composite_reference.loss_mirror_error, not one signed difference;
* cap on undecidable rays: a ray is left out of the gated comparisons (draw) only when a pre-clip channel of the float64 reference
  lies within 1e-5 of 0 or 1 without being on it; at most 2 % of a case's rays, and none of classes 1 (all sigma zero), 7 (rgb
  outside [0, 1]) and 8 (target = own pixel);
* power: every mutant of composite_reference.MUTANTS is more than 10 x tol away from the reference in at least one checked output
  on at least one case.  `pytest -s` prints the table.

Known limit: replacing `ex` by `x` in dsigma (x = ex + 1e-10) moves dsigma by at most 3e-8 of a ray's largest element and cannot be
told apart; it is not among the mutants and no test claims it.

The float32 oracle is NOT the yardstick: its render_backward forms Q = rev - prod, which behind an opaque sample cancels to rounding
noise and is then divided by x = 1e-10, so its dalpha there is wrong by orders of magnitude.  (In dsigma = dalpha delta ex the factor
ex <= x takes the noise back down: on the cases of this file its dsigma stays within 1.1e-5 of a ray's maximum, about what mirror32
reaches.  A float32 computation cannot bound another one either way.)  The kernel and mirror32() build a true exclusive suffix sum.
"""
import numpy as np
import pytest

from oracle import nerf_oracle as O
from tests import composite_reference as CR

CHECKED = ("image", "depth", "weights", "draw", "last", "loss")


def test_templates_full_and_ragged_and_limits():
    """the sample counts reach every composite_kernel<C>, each with a full and a ragged last lane, and both limits"""
    by_c = {}
    for S in CR.S_CASES:
        by_c.setdefault(CR.template_C(S), []).append(S)
    assert sorted(by_c) == [1, 2, 3, 4, 8, 12, 16]
    for C, sizes in by_c.items():
        assert any(S == 64 * C for S in sizes) and any(S % C or S < 64 * C for S in sizes), (C, sizes)
    assert min(CR.S_CASES) == 2 and max(CR.S_CASES) == 1024 and CR.R_CASE % 4 == 1


@pytest.mark.parametrize("S,white", CR.CASES)
def test_inputs_hold_what_the_classes_promise(S, white):
    c = CR.case(S, white)
    cls, raw, t, ref = c["cls"], c["raw"], c["t"], c["ref"]
    assert sorted(set(cls)) == list(range(1, CR.N_CLASSES + 1))
    z = cls == CR.ALL_ZERO
    assert not raw[z, :, 3].any() and (ref["pre"][z] == (1.0 if white else 0.0)).all()          # exactly on the gate's edge: open
    assert not ref["weights"][z].any() and not ref["draw"][z, :, :3].any() and (ref["draw"][z, :, 3] != 0).all()
    out = cls == CR.RGB_OUTSIDE
    assert ((ref["pre"][out] < -0.1) | (ref["pre"][out] > 1.1)).all() and not ref["draw"][out].any()
    assert not ref["draw"][cls == CR.OWN_PIXEL].any()
    op = cls == CR.OPAQUE
    if S >= 64:
        assert (ref["weights"][op].sum(axis=1) > 0.99).all()                                     # an opaque front ...
        x = np.float32(1.0) - (np.float32(1.0) - np.exp(-(raw[op, :-1, 3] * np.diff(t[op], axis=1)).astype(np.float64)).astype(np.float32)) + np.float32(1e-10)
        assert (x.min(axis=1) == np.float32(1e-10)).all()                                        # ... with x == 1e-10 exactly
    d = np.diff(t, axis=1)
    assert (d[cls == CR.UNSORTED] < 0).any(axis=1).all() and (np.abs(raw[cls == CR.UNSORTED, :-1, 3] * d[cls == CR.UNSORTED]) <= 5).all()
    assert (d[cls == CR.REPEATED_T] == 0).any(axis=1).all()
    sorted_cls = ~np.isin(cls, (CR.UNSORTED,))
    assert (d[sorted_cls] >= 0).all()
    rgb = raw[cls != CR.RGB_OUTSIDE, :, :3]
    assert rgb.min() > 0.02 - 1e-6 and rgb.max() < 0.98 + 1e-6


@pytest.mark.parametrize("S,white", CR.CASES)
def test_reference_in_float64_is_the_oracle(S, white):
    c = CR.case(S, white)
    raw, t, tgt = c["raw"].astype(np.float64), c["t"].astype(np.float64), c["target"].astype(np.float64)
    gs, ls = c["grad_scale"], c["loss_scale"]
    ref = CR.reference(raw, t, tgt, white, gs, ls)
    img, depth, w, cache = O.render_image_depth_chunk(raw[..., :3], raw[..., 3], t, bool(white), want_cache=True)
    drgb, dsigma = O.render_backward(cache, gs * (img - tgt))
    for got, want in ((ref["image"], img), (ref["depth"], depth), (ref["weights"], w), (ref["pre"], cache["pre"])):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)
    assert abs(ref["loss"] - ls * np.sum((img - tgt) ** 2)) < 1e-14
    # the oracle's Q = rev - prod carries 1e-16 |rev| / x into dalpha even in float64; delta ex scales it back to 1e-16 |rev| delta
    scale = np.abs(ref["draw"]).reshape(len(t), -1).max(axis=1)[:, None]
    np.testing.assert_allclose(ref["draw"][..., :3], drgb, rtol=1e-12, atol=1e-18)
    assert (np.abs(ref["draw"][..., 3] - dsigma) <= 1e-9 * scale).all()


@pytest.mark.parametrize("S,white", CR.CASES)
def test_tolerance_and_cap_on_undecidable_rays(S, white):
    c = CR.case(S, white)
    skip, cls = c["skip"], c["cls"]
    print(f"\nS {S:4d} white {white}: undecidable rays {int(skip.sum())} of {len(skip)}   mirror error / tol")
    for k in CHECKED:
        print(f"    {k:8s} numpy exp {c['mirror_errs']['numpy'][k]:.3e}  jittered exp {c['mirror_errs']['jitter'][k]:.3e}  tol {c['tol'][k]:.3e}")
    assert skip.sum() <= 0.02 * len(skip)
    assert not skip[np.isin(cls, (CR.ALL_ZERO, CR.RGB_OUTSIDE, CR.OWN_PIXEL))].any()
    # recomputed here from the pre-clip image alone
    p = c["ref"]["pre"]
    near = ((np.abs(p) < 1e-5) & (p != 0)) | ((np.abs(p - 1) < 1e-5) & (p != 1))
    assert np.array_equal(skip, near.any(axis=1))
    for k in CHECKED:
        assert 0 < c["tol"][k] < 1e-2, (k, c["tol"][k])
    assert c["tol"]["weights"] < 5e-5 and c["tol"]["image"] < 1e-4


def mutant_table():
    """{mutant: [(error / tol of the output that shows it best, that output, case) for every case]}"""
    table = {m: [] for m in CR.MUTANTS}
    for S, white in CR.CASES:
        c = CR.case(S, white)
        for m in CR.MUTANTS:
            out = CR.reference(c["raw"], c["t"], c["target"], white, c["grad_scale"], c["loss_scale"], own_pixel=c["own"], loss0=CR.LOSS0, mutant=m)
            e = CR.errors(out, c["ref"], c["skip"])
            k = max(CHECKED, key=lambda k: e[k] / c["tol"][k])
            table[m].append((e[k] / c["tol"][k], k, (S, white)))
    return table


def test_every_mutant_is_far_outside_the_tolerance():
    table = mutant_table()
    print("\nerror / tol of the output that shows the mutant best (inf: not finite, or non-zero where the reference is exactly zero)")
    print("mutant                      best case                       weakest case                   cases above 10 x tol")
    for m, rows in table.items():
        hi, lo = max(rows), min(rows)
        n = sum(r[0] > CR.POWER_FACTOR for r in rows)
        print(f"    {m:24s} {hi[0]:9.3g} {hi[1]:8s} {str(hi[2]):10s}   {lo[0]:9.3g} {lo[1]:8s} {str(lo[2]):10s}   {n} of {len(rows)}")
    for m, rows in table.items():
        assert max(rows)[0] > CR.POWER_FACTOR, (m, max(rows))
        # ... and in fact on EVERY case where the mistake can show at all: the background term needs the white background, and at
        # S = 2 the only later sample is the last one, whose alpha = 1 - exp(-sigma 1e-10) is zero (nothing to carry)
        for ratio, k, (S, white) in rows:
            if (m == "white_gsum_dropped" and not white) or (m == "no_lane_carry" and S == 2):
                continue
            assert ratio > CR.POWER_FACTOR, (m, S, white, ratio)


def test_weakest_case_of_the_lane_carry_mutant():
    """a suffix sum that drops the carry from later lanes is caught at EVERY sample count but 2"""
    for S, white in CR.CASES:
        if S == 2:          # two lanes, but the last sample has alpha = 1 - exp(-sigma 1e-10) = 0: it carries nothing to the first
            continue
        c = CR.case(S, white)
        out = CR.reference(c["raw"], c["t"], c["target"], white, c["grad_scale"], c["loss_scale"], own_pixel=c["own"], loss0=CR.LOSS0, mutant="no_lane_carry")
        e = CR.errors(out, c["ref"], c["skip"])
        assert e["draw"] > CR.POWER_FACTOR * c["tol"]["draw"], (S, white, e["draw"], c["tol"]["draw"])


def test_mirror_zero_classes_are_exactly_zero():
    """classes 7 and 8 and the drgb of class 1: every draw element of the float32 mirror is zero, as the kernel's must be"""
    for S, white in ((65, 0), (512, 1)):
        c = CR.case(S, white)
        m = CR.mirror32(c["raw"], c["t"], c["target"], white, c["grad_scale"], c["loss_scale"], own_pixel=c["own"])
        assert (m["draw"][np.isin(c["cls"], (CR.RGB_OUTSIDE, CR.OWN_PIXEL))] == 0).all()
        assert (m["draw"][c["cls"] == CR.ALL_ZERO, :, :3] == 0).all() and (m["draw"][c["cls"] == CR.ALL_ZERO, :, 3] != 0).all()
        assert np.array_equal(CR.dead_tiles(m["draw"][:, :S // 32 * 32], c["raw"][:, :S // 32 * 32]).reshape(len(c["cls"]), -1)[c["cls"] == CR.ALL_ZERO].any(), False)


def test_ex_for_x_in_dsigma_is_not_distinguishable():
    """the known limit: dsigma = dalpha delta x instead of ... ex differs by dalpha delta 1e-10"""
    worst = 0.0
    for S, white in ((64, 0), (1024, 1)):
        c = CR.case(S, white)
        ref = c["ref"]
        raw, t = c["raw"], c["t"]
        delta = np.concatenate([np.diff(t, axis=1), np.full((len(t), 1), np.float32(1e-10))], axis=1).astype(np.float64)
        ex = np.exp(-(raw[..., 3] * delta.astype(np.float32)).astype(np.float64)).astype(np.float32).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(ex > 0, ref["draw"][..., 3] / ex * 1e-10, 0.0)             # = dalpha delta 1e-10
        scale = np.abs(ref["draw"]).reshape(len(t), -1).max(axis=1)
        ok = (scale > 0) & ~c["skip"]
        worst = max(worst, float((np.abs(d).max(axis=1)[ok] / scale[ok]).max()))
    assert worst < c["tol"]["draw"]
