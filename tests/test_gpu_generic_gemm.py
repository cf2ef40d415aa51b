"""csrc/generic.hip's four matmul kernels, each launched on its own on caller-made buffers (knerf_debug_generic_gemm /
knerf_debug_generic_wgrad) against the float64 reference of tests/generic_gemm_reference.py: gemm_ws_kernel<1|2|4|8> (also its
second persistent iteration and its column-block mapping), the streaming gemm_kernel<1|2|4|8>, wgrad_coop_kernel and the per-wave
wgrad_kernel, with wgrad_reduce_kernel behind both in deterministic mode.

Exact family (small integers as bf16; every fp32 partial sum exact in any order): every comparison is == on bits.  Real-valued family:
fp32 results within n 2^-23 (sum |a b| + |bias or prefill|), bf16 results within that plus half a bf16 ulp; relu bits against the
device's OWN stored value.  Cases, inputs and bounds are the reference module's; tests/test_generic_gemm_host.py proves on the CPU
that these inputs see each of the reference's mutants and that the case tables close over the launch classes the product reaches.
Outputs sit inside wider buffers whose guard columns, guard rows and dead tiles are prefilled and must come back untouched; operand
padding and the rows of dead tiles hold bf16 NaN.  Each test prints its worst error / bound ratio per kernel (pytest -s);
tests/README.md records them."""
import numpy as np
import pytest
import torch

from tests import generic_gemm_reference as R

pytestmark = pytest.mark.gpu

SENT_F = np.float32(12345.678)
_CACHE = {}


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def host16(t):
    return t.cpu().numpy().view(np.uint16)


def report(kernel, ratio):
    print(f"\nRATIO {kernel} {ratio:.4f}")


def gemm_case(K, N, M, family):
    key = ("g", K, N, M, family)
    if key not in _CACHE:
        _CACHE.clear()                                      # one case's operands at a time
        c = R.gemm_inputs(K, N, M, family)
        c["A_bits"], c["Bt_dev"] = R.padded_bits(c["A"], c["lda"]), dev(R.padded_bits(c["Bt"], c["ldb"]))
        c["A_dev"], c["bias_dev"] = dev(c["A_bits"]), dev(c["bias"])
        _CACHE[key] = c
    return _CACHE[key]


def a_with_dead_rows(c, live):
    """A on the device; with a live list the rows of every other tile are bf16 NaN"""
    if live is None:
        return c["A_dev"]
    A = c["A_bits"].copy()
    A[~R._live_rows(c["M"], live)] = R.NAN_BF16
    return dev(A)


def launch_gemm(c, mode, live=None, mask_in=None):
    """one launch; returns (Cb uint16 [M + 32][ldc] | None, Cf float32 [M + 32][ldcf] | None, mask_out tensor | None)"""
    from keras_nerf_amd import debug
    K, N, M = c["K"], c["N"], c["M"]
    tiles = M // 32
    Cb = Cf = mo = None
    kw = {}
    if mode == "head":
        Cf = torch.full(((M + 32) * c["ldcf"],), float(SENT_F), device="cuda")
        kw = dict(bias=c["bias_dev"], n_real=c["n_real"], Cf=Cf, ldcf=c["ldcf"])
    else:
        Cb = dev(np.full((M + 32) * c["ldc"], R.SENT_C, np.uint16))
        kw = dict(Cb=Cb, ldc=c["ldc"], c_col0=c["c_col0"])
        if mode == "dgrad":
            kw.update(mask_in=mask_in, mask_cols=c["mask_cols"])
        else:
            kw.update(bias=c["bias_dev"], n_real=c["n_real"], relu=mode == "forward")
            if mode == "forward":
                mo = torch.full(((tiles + 1) * c["mask_cols"] * 32,), R.SENT_MASK, dtype=torch.uint8, device="cuda")
                kw.update(mask_out=mo, mask_cols=c["mask_cols"])
    debug.generic_gemm(a_with_dead_rows(c, live), c["lda"], c["Bt_dev"], c["ldb"], M, N, K, live=live, **kw)
    torch.cuda.synchronize()
    return (None if Cb is None else host16(Cb).reshape(M + 32, c["ldc"]), None if Cf is None else Cf.cpu().numpy().reshape(M + 32, c["ldcf"]), mo)


def check_cb(c, got, ref, kernel):
    """guards untouched; body bit-equal (exact) or inside the derived bound (real-valued); returns the body's bit patterns"""
    N, M, c0 = c["N"], c["M"], c["c_col0"]
    assert (got[:, :c0] == R.SENT_C).all() and (got[:, c0 + N:] == R.SENT_C).all() and (got[M:] == R.SENT_C).all()
    body = got[:M, c0:c0 + N]
    t = ref["touched"]
    assert (body[~t] == R.SENT_C).all()                                # dead tiles: untouched
    if c["family"] == "exact":
        bad = np.argwhere(body != R.expected_cb(ref))
        assert len(bad) == 0, (len(bad), bad[:8].tolist())
        return body
    val = R.from_bits(body[t]).astype(np.float64)
    assert np.isfinite(val).all()
    rv, rb = ref["value"][t], ref["bound"][t]
    tol = rb + R.half_ulp_bf16(np.abs(rv) + rb)
    err = np.abs(val - rv)
    if t.any():
        report(kernel, float((err / tol).max()))
    assert (err <= tol).all(), float((err / tol).max())
    return body


def check_mask(c, mo, body, ref):
    """the stored relu bits against the activation THIS launch stored: bit <=> stored bf16 > 0, for every element"""
    N, M = c["N"], c["M"]
    m = mo.cpu().numpy().reshape(M // 32 + 1, c["mask_cols"], 32)
    assert (m[M // 32:] == R.SENT_MASK).all() and (m[:, N // 8:] == R.SENT_MASK).all()
    bits = R.mask_unpack(m[:M // 32], N)
    assert np.array_equal(bits, R.from_bits(body) > 0)
    if c["family"] == "exact":
        assert np.array_equal(bits, ref["bits"])
    return bits


GEMM_PARAMS = [(K, N, M, cls, fam) for K, N, M, cls in R.GEMM_CASES for fam in ("exact", "real") if fam == "exact" or M <= R.LARGE_M]


@pytest.mark.parametrize("K,N,M,cls,family", GEMM_PARAMS, ids=[f"{p[0]}x{p[1]}x{p[2]}-{p[4]}" for p in GEMM_PARAMS])
def test_gemm_against_fp64(K, N, M, cls, family):
    from keras_nerf_amd import debug
    d = debug.gemm_launch(M, N, K)
    assert R.gemm_class(d) == cls                                      # the instantiation this row is about
    kernel = f"gemm_{d['kernel']}<{d['nt']}>"
    c = gemm_case(K, N, M, family)
    large = M > R.LARGE_M
    # forward: bias, relu, relu bits out; Cb at a column offset inside a wider buffer
    ref = R.gemm_reference(c, "forward")
    cb, _, mo = launch_gemm(c, "forward")
    body = check_cb(c, cb, ref, kernel)
    check_mask(c, mo, body, ref)
    cb, _, _ = launch_gemm(c, "norelu")
    check_cb(c, cb, R.gemm_reference(c, "norelu"), kernel)
    if not large:
        # fp32 output (the head form where N = 32: n_real = 4)
        ref_h = R.gemm_reference(c, "head")
        _, cf, _ = launch_gemm(c, "head")
        assert (cf[M:] == SENT_F).all() and (cf[:, N:] == SENT_F).all()
        if family == "exact":
            assert np.array_equal(cf[:M, :N].view(np.uint32), ref_h["value"].astype(np.float32).view(np.uint32))
        else:
            err = np.abs(cf[:M, :N].astype(np.float64) - ref_h["value"])
            ok = ref_h["bound"] > 0
            assert (err[~ok] == 0).all()
            report(kernel + "/fp32", float((err[ok] / ref_h["bound"][ok]).max()))
            assert (err <= ref_h["bound"]).all()
    # dgrad: relu bits in -- reference-built, and the ones the forward launch above stored; dead-tile lists
    ref_mask = dev(R.mask_pack(c["mask_bits"], c["mask_cols"]).reshape(-1))
    own_bits = R.mask_unpack(mo.cpu().numpy().reshape(M // 32 + 1, c["mask_cols"], 32)[:M // 32], N)
    if large:           # "most": more list entries than one pass of the persistent grid has waves
        assert len(c["lists"]["most"]) > 8 * d["gx"]
    every = ("none", "empty", "one", "third", "shuffled", "most")
    # (the large rows compare tens of millions of elements per launch: the lists that differ in kind, the own bits once)
    for mk, bits, names in ((ref_mask, c["mask_bits"], ("none", "third", "most") if large else every), (mo, own_bits, ("none",) if large else every)):
        for name in names:
            live = c["lists"][name]
            cb, _, _ = launch_gemm(c, "dgrad", live=live, mask_in=mk)
            ref = R.gemm_reference(c, "dgrad", live=live, mask_bits=bits)
            assert name != "empty" or not ref["touched"].any()
            check_cb(c, cb, ref, kernel + "/dgrad")


def test_relu_bits_cross_two_column_widths():
    """the writer and the reader of the bits hold different numbers of features per lane: forward 320 -> 256 is gemm_ws_kernel<4>
    (gy = 2), the dgrad 256 -> 256 over the same features is gemm_ws_kernel<8>"""
    from keras_nerf_amd import debug
    assert debug.gemm_launch(384, 256, 320)["nt"] == 4 and debug.gemm_launch(384, 256, 256)["nt"] == 8
    for family in ("exact", "real"):
        cf = gemm_case(320, 256, 384, family)
        cb, _, mo = launch_gemm(cf, "forward")
        body = check_cb(cf, cb, R.gemm_reference(cf, "forward"), "gemm_ws<4>")
        bits = check_mask(cf, mo, body, R.gemm_reference(cf, "forward"))
        mo = mo.clone()
        cd = gemm_case(256, 256, 384, family)
        assert cd["mask_cols"] == cf["mask_cols"]
        for name in ("none", "third"):
            live = cd["lists"][name]
            cb, _, _ = launch_gemm(cd, "dgrad", live=live, mask_in=mo)
            check_cb(cd, cb, R.gemm_reference(cd, "dgrad", live=live, mask_bits=bits), "gemm_ws<8>/dgrad")


# ---- weight gradients -------------------------------------------------------------------------------------------------------
def wgrad_case(case, family):
    K, N, steps, segs, n_real, _ = case
    key = ("w", K, N, steps, family)
    if key not in _CACHE:
        _CACHE.clear()
        c = R.wgrad_inputs(K, N, steps, segs, n_real, family)
        c["X_bits"], c["Z_bits"] = R.padded_bits(c["X"], c["ldx"]), R.padded_bits(c["Z"], c["ldz"])
        _CACHE[key] = c
    return _CACHE[key]


def launch_wgrad(c, det, live, per_wave, dead="nan"):
    """one launch on a fresh copy of the prefilled gradient; rows of dead tiles: NaN in both operands, or (dead="zero") dZ = 0"""
    from keras_nerf_amd import debug
    X, Z = c["X_bits"], c["Z_bits"]
    if live is not None:
        deadrows = ~R._live_rows(c["M"], live)
        X, Z = X.copy(), Z.copy()
        if dead == "nan":
            X[deadrows] = R.NAN_BF16
            Z[deadrows] = R.NAN_BF16
        else:
            Z[deadrows] = 0
    grad = dev(c["grad0"].copy())
    partial = None
    if det:             # every slab element the reduce pass reads must have been written by its unit: the arena starts as NaN
        partial = torch.full((debug.wgrad_partial_floats(c["K"], c["N"], per_wave),), float("nan"), device="cuda")
    debug.generic_wgrad(dev(X), c["ldx"], dev(Z), c["ldz"], c["steps"], c["K"], c["N"], grad, c["w_off"], c["b_off"], c["n_real"], c["segs"],
                        partial=partial, live=live, per_wave=per_wave)
    torch.cuda.synchronize()
    return grad.cpu().numpy()


def check_grad(c, got, ref, kernel):
    g0 = c["grad0"]
    w = ref["written"]
    assert np.array_equal(got[~w].view(np.uint32), g0[~w].view(np.uint32))           # guards around the kernel and the bias
    if c["family"] == "exact":
        bad = np.nonzero(got.view(np.uint32) != ref["grad"].astype(np.float32).view(np.uint32))[0]
        assert len(bad) == 0, (len(bad), bad[:8].tolist())
        return
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref["grad"])[w]
    report(kernel, float((err / ref["bound"][w]).max()))
    assert (err <= ref["bound"][w]).all(), float((err / ref["bound"][w]).max())


WGRAD_PARAMS = [(i, pw, fam) for i in range(len(R.WGRAD_CASES)) for pw in (False, True) if not pw or i in R.PER_WAVE_ROWS for fam in ("exact", "real")]


@pytest.mark.parametrize("row,per_wave,family", WGRAD_PARAMS,
                         ids=[f"{R.WGRAD_CASES[i][0]}x{R.WGRAD_CASES[i][1]}x{R.WGRAD_CASES[i][2]}-{'wave' if pw else 'product'}-{f}" for i, pw, f in WGRAD_PARAMS])
def test_wgrad_against_fp64(row, per_wave, family):
    from keras_nerf_amd import debug
    case = R.WGRAD_CASES[row]
    K, N, steps, segs, n_real, want = case
    d = debug.wgrad_launch(K, N, steps, per_wave=per_wave)
    if per_wave:
        assert d["kernel"] == "wave"
        kernel = f"wgrad_wave<{d['kt']},{d['nt']}>"
    else:
        assert d["kernel"] == "coop" and (d["gx"], d["gy"], d["gz"]) == want[:3]
        kernel = "wgrad_coop"
    c = wgrad_case(case, family)
    atomic = {}
    for det in (False, True):
        for name in ("none", "empty", "one", "third") + (() if det else ("shuffled",)):
            live = c["lists"][name]
            ref = R.wgrad_reference(c, live=live, gx=d["gx"])
            got = launch_wgrad(c, det, live, per_wave)
            check_grad(c, got, ref, kernel + ("/det" if det else ""))
            if not det:
                atomic[name] = got
            else:
                # deterministic mode: a second launch gives the same bits; exact family: the same bits as atomic mode
                again = launch_wgrad(c, det, live, per_wave)
                assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), name
                if family == "exact":
                    assert np.array_equal(got.view(np.uint32), atomic[name].view(np.uint32)), name
    # deterministic mode, dZ exactly zero on the dead tiles: walking the list forms the same sums in the same order as walking every
    # tile (csrc/generic.hip unit_schedule) -- bit-identical also in the real-valued family
    live = c["lists"]["third"]
    with_list = launch_wgrad(c, True, live, per_wave, dead="zero")
    c2 = dict(c)
    Zz = c["Z_bits"].copy()
    Zz[~R._live_rows(c["M"], live)] = 0
    c2["Z_bits"] = Zz
    without = launch_wgrad(c2, True, None, per_wave)
    assert np.array_equal(with_list.view(np.uint32), without.view(np.uint32))
    check_grad(c, with_list, R.wgrad_reference(c, live=live, gx=d["gx"]), kernel + "/det")
