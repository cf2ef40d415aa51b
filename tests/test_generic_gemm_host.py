"""CPU side of the operator-level tests of csrc/generic.hip's GEMM and weight-gradient launchers (tests/test_gpu_generic_gemm.py):

* coverage closure: every launch class -- (kernel, NT, gy > 1, more than one tile per wave) of a GEMM, (kernel, gx gy > 1, idle units,
  schedule-length class) of a weight gradient -- that the general-shape contexts of the suite reach (tests/test_gpu_generic.py SHAPES,
  the default shape, 288 and 288 -> 384 of tests/test_width_padding.py; coarse and fine pass of their 256-ray problems) is reached by a
  row of the GPU case tables, and so are the classes the product can reach but the suite never does: the streaming GEMM at every NT and
  the second persistent iteration at gy = 1 and 2;
* the mutants of tests/generic_gemm_reference.py differ from the reference on every case where they can show: the cases' inputs are
  not blind to these bugs;
* the two entry points refuse bad arguments (the check they run before any HIP call).
No device is touched: the launch description is host arithmetic and the argument check reads nothing behind the device pointers."""
import ctypes as C

import numpy as np
import pytest

from keras_nerf_amd import _lib, debug
from tests import generic_gemm_reference as R

SUITE_SHAPES = {            # (n_layers, dense_units, skip_layer, pos_emb_xyz, pos_emb_dir): tests/test_gpu_generic.py SHAPES, then the others
    "small_skip2": (4, 128, 2, 6, 2), "skip1_every_layer": (3, 64, 1, 4, 1), "odd_units": (2, 96, 4, 10, 4), "wide_enc": (5, 160, 3, 12, 5),
    "tiny32": (8, 32, 4, 4, 2), "deep_wide": (12, 512, 5, 10, 4), "no_encoding": (1, 2, 1, 0, 0),
    "default": (8, 256, 4, 10, 4), "width_288": (3, 288, 2, 10, 4), "width_288_padded": (3, 384, 2, 10, 4),
}
SUITE_ROWS = (256 * 64, 256 * (64 + 128))       # coarse and fine pass of the suite's 16 x 16 image, n_coarse 64, n_fine 128


def test_suite_shape_list_is_the_one_of_the_whole_network_tests():
    import ast
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    tree = ast.parse(open(os.path.join(here, "test_gpu_generic.py")).read())
    shapes = next(ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) and n.targets[0].id == "SHAPES")
    assert all(SUITE_SHAPES[k] == v for k, v in shapes.items()) and len(shapes) == 7


def plan_rows(shape):
    nl, u, sk, lx, ld = shape
    cfg = _lib.KnerfConfig(64, 128, lx, ld, nl, u, sk, 0, 0, 1e-3, 0.9, 0.999, 1e-7)
    n = C.c_size_t(0)
    dbg = debug.load()
    assert dbg.knerf_debug_generic_plan(C.byref(cfg), None, C.byref(n)) == 0
    buf = (C.c_int32 * n.value)()
    assert dbg.knerf_debug_generic_plan(C.byref(cfg), buf, C.byref(n)) == 0
    return np.array(buf[:]).reshape(-1, 16), nl


def product_launches(shape):
    """(gemm (N, K) list, wgrad (K, N) list) of one forward + backward of a general-shape context (csrc/generic.hip run_layers / backward)"""
    rows, nl = plan_rows(shape)
    up = int(rows[0][5])
    head_K = int(rows[nl - 1][15])
    gemms = [(int(r[5]), int(r[4])) for r in rows[:nl]] + [(32, head_K)]              # forward: trunk layers, composed head
    gemms += [(up, 32)] + [(up, up)] * (nl - 1)                                        # dgrad: head, then every trunk layer but the first
    wgrads = [(int(r[4]), int(r[5])) for r in rows[:nl]] + [(head_K, 32)]
    return gemms, wgrads


def coarse_gemm_class(d):
    return (d["kernel"], d["nt"], d["gy"] > 1, d["tiles_per_wave"] > 1)


def wgrad_classes(d, steps):
    k, multi, idle, sched = R.wgrad_class(d, steps)
    return {(k, multi, idle, s) for s in sched}


def test_case_tables_reach_their_named_classes():
    for K, N, M, want in R.GEMM_CASES:
        d = debug.gemm_launch(M, N, K)
        assert R.gemm_class(d) == want, (K, N, M, d)
    for K, N, steps, segs, n_real, want in R.WGRAD_CASES:
        d = debug.wgrad_launch(K, N, steps)
        assert d["kernel"] == "coop"                     # what the product picks for every layer
        counts = [c for det in (False, True) for c in R.unit_counts(steps, d["units"], det)]
        assert (d["gx"], d["gy"], d["gz"], min(counts), max(counts)) == want, (K, N, steps, d, min(counts), max(counts))
    # selector 1: the per-wave kernel's instantiations <1,1>, <2,2> and <2,1>
    inst = {(lambda d: (d["kernel"], d["kt"], d["nt"]))(debug.wgrad_launch(*R.WGRAD_CASES[i][:3], per_wave=True)) for i in R.PER_WAVE_ROWS}
    assert inst == {("wave", 1, 1), ("wave", 2, 2), ("wave", 2, 1)}


def test_coverage_closure():
    have_g = {coarse_gemm_class(debug.gemm_launch(M, N, K)) for K, N, M, _ in R.GEMM_CASES}
    have_w = set()
    for K, N, steps, *_ in R.WGRAD_CASES:
        have_w |= wgrad_classes(debug.wgrad_launch(K, N, steps), steps)
    need_g, need_w = {}, {}
    for name, shape in SUITE_SHAPES.items():
        gemms, wgrads = product_launches(shape)
        for M in SUITE_ROWS:
            for N, K in gemms:
                need_g.setdefault(coarse_gemm_class(debug.gemm_launch(M, N, K)), (name, M, N, K))
            for K, N in wgrads:
                for cls in wgrad_classes(debug.wgrad_launch(K, N, M // 32), M // 32):
                    need_w.setdefault(cls, (name, M, K, N))
    missing = {c: w for c, w in need_g.items() if c not in have_g}
    assert not missing, f"GEMM classes the suite's contexts reach and the case table does not: {missing}"
    missing = {c: w for c, w in need_w.items() if c not in have_w}
    assert not missing, f"weight-gradient classes the suite's contexts reach and the case table does not: {missing}"
    # what the product can reach and no whole-network test does
    exact = {R.gemm_class(debug.gemm_launch(M, N, K)) for K, N, M, _ in R.GEMM_CASES}
    for nt in (1, 2, 4, 8):
        assert ("stream", nt, 1, 1) in exact
    assert any(c[0] == "ws" and c[2] == 1 and c[3] == 2 for c in exact) and any(c[0] == "ws" and c[2] == 2 and c[3] == 2 for c in exact)
    # dense_units >= 2,400 is how the public API gets to the streaming kernel
    assert debug.gemm_launch(128, 2400, 2400)["kernel"] == "stream" and debug.gemm_launch(128, 2368, 2368)["kernel"] == "ws"


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def _window(M):
    """the rows the CPU test evaluates: everything, or the last 256 rows of a large case (the second persistent iteration's tiles)"""
    return None if M <= R.LARGE_M else slice(M - 256, M)


def _differs(c, ref, mut, mode):
    """does the mutant show?  exact family: any differing bit of the output (or of the relu bits); real-valued family: any element
    further from the reference than the device may be"""
    if mode == "forward" and np.any(ref["bits"] != mut["bits"]):
        return True
    if np.any(ref["touched"] != mut["touched"]):
        return True
    if c["family"] == "exact":
        return bool(np.any(R.expected_cb(ref) != R.expected_cb(mut)))
    tol = ref["bound"] + R.half_ulp_bf16(np.abs(ref["value"]) + ref["bound"])
    return bool(np.any(np.abs(ref["value"] - mut["value"]) > 2 * tol))


GEMM_PARAMS = [(K, N, M, cls, fam) for K, N, M, cls in R.GEMM_CASES for fam in ("exact", "real") if fam == "exact" or M <= R.LARGE_M]


@pytest.mark.parametrize("K,N,M,cls,family", GEMM_PARAMS, ids=[f"{p[0]}x{p[1]}x{p[2]}-{p[4]}" for p in GEMM_PARAMS])      # the large rows: exact only
def test_gemm_mutants_show_on_every_case(K, N, M, cls, family):
    c = R.gemm_inputs(K, N, M, family)
    rows, nt = _window(M), cls[1]
    last = M // 32 - 1
    lists = [None] if M > R.LARGE_M else [None, c["lists"]["third"]]
    shown = set()
    for mode in ("forward", "norelu", "dgrad"):
        for live in lists:
            victim = last if live is None else int(live[0])
            kw = dict(live=live, mask_bits=c["mask_bits"], rows=rows, nt=nt)
            ref = R.gemm_reference(c, mode, **kw)
            for m in R.GEMM_MUTANTS:
                can = {"col_assign": nt > 1, "k_tail": K % 64 != 0, "skip_tile": True, "bias_pad": mode != "dgrad",
                       "mask_natural": mode == "dgrad",
                       "bit_pre_round": False}[m]     # a positive fp32 normal never rounds to a bf16 zero: see the test below
                if not can:
                    continue
                mut = R.gemm_reference(c, mode, mutant=m, victim=victim, **kw)
                assert _differs(c, ref, mut, mode), (m, mode, live is not None)
                shown.add(m)
    assert shown >= {"skip_tile", "bias_pad", "mask_natural"}


def test_relu_bit_before_rounding_shows_only_below_the_normal_range():
    """The bit is what a reader of the STORED bf16 value decides.  A positive fp32 value rounds to a bf16 zero only below 2^-134,
    far inside the subnormal range that is outside the contract, so no case of the tables can tell the two rules apart; this pins that
    the reference implements the documented one, with an accumulator a bias cancels down to 2^-140."""
    c = R.gemm_inputs(32, 32, 128, "real")
    c["n_real"] = 32
    c["bias"][1] = np.float32(2.0 ** -140)               # row 5, column 1: accumulator exactly 0 (gemm_inputs)
    ref, mut = R.gemm_reference(c, "forward"), R.gemm_reference(c, "forward", mutant="bit_pre_round")
    assert not ref["bits"][5, 1] and mut["bits"][5, 1] and ref["value"][5, 1] > 0
    assert (ref["bits"] != mut["bits"]).sum() == np.sum(c["bias"][1] == ref["value"][:, 1])


def test_real_family_has_its_edge_values_and_no_subnormal_result():
    for K, N, M, _ in R.GEMM_CASES:
        if M > R.LARGE_M:
            continue
        c = R.gemm_inputs(K, N, M, "real")
        ref = R.gemm_reference(c, "forward")
        v = ref["value"]
        assert v[5, 0] == 0.0 and not ref["bits"][5, 0]                                   # cancelled to exactly zero
        assert v[5, 1] == R.TINY and ref["bits"][5, 1] and R.to_bits(np.float32(v[5, 1])) == 0x0080
        for mode in ("forward", "norelu"):
            v = np.abs(R.gemm_reference(c, mode)["value"])
            assert not np.any((v > 0) & (v < R.TINY))
        assert 0.15 < (c["A"] == 0).mean() < 0.25 and 0.15 < (c["Bt"] == 0).mean() < 0.25


def test_mask_layout_round_trip_and_documented_byte_order():
    rng = np.random.default_rng(0)
    bits = rng.random((64, 48)) < 0.5
    m = R.mask_pack(bits, 7)
    assert m.shape == (2, 7, 32) and (m[:, 6] == R.SENT_MASK).all()
    assert np.array_equal(R.mask_unpack(m, 48), bits)
    for hh in range(2):
        for i in range(16):
            row = (i & 3) + 8 * (i >> 2) + 4 * hh
            for tile in range(2):
                for f in (0, 9, 47):
                    assert (m[tile, f // 8, 16 * hh + i] >> (f % 8)) & 1 == bits[tile * 32 + row, f]


@pytest.mark.parametrize("family", ["exact", "real"])
@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in R.WGRAD_CASES])
def test_wgrad_mutants_show_on_every_case(case, family):
    K, N, steps, segs, n_real, _ = case
    c = R.wgrad_inputs(K, N, steps, segs, n_real, family)
    gx = debug.wgrad_launch(K, N, steps)["gx"]
    two_seg_gap = len(segs) == 2 and segs[1][0] > segs[0][0] + segs[0][1]
    for live in (None, c["lists"]["third"]):
        victim = steps - 1 if live is None else int(live[-1])
        ref = R.wgrad_reference(c, live=live, gx=gx)
        for m in R.WGRAD_MUTANTS:
            can = {"seg_pad": two_seg_gap, "bias_block": gx > 1}.get(m, True)
            if family == "real" and steps > 100 and m in ("skip_tile", "dup_tile"):
                continue        # one step in hundreds is inside n 2^-23 sum |x z|: only the exact family sees it there
            if not can:
                continue
            mut = R.wgrad_reference(c, live=live, gx=gx, mutant=m, victim=victim)
            if family == "exact":
                assert np.any(ref["grad"].astype(np.float32).view(np.uint32) != mut["grad"].astype(np.float32).view(np.uint32)), m
            else:
                assert np.any(np.abs(ref["grad"] - mut["grad"]) > 2 * ref["bound"]), m
    # guards: what no kernel row and no bias maps to
    assert (~ref["written"]).sum() >= 9


def test_the_table_has_a_case_for_every_mutant():
    assert any(c[3][1] > 1 for c in R.GEMM_CASES) and any(c[0] % 64 for c in R.GEMM_CASES)
    assert any(len(c[3]) == 2 and c[3][1][0] > c[3][0][1] for c in R.WGRAD_CASES)
    assert any(debug.wgrad_launch(c[0], c[1], c[2])["gx"] > 1 for c in R.WGRAD_CASES)


# ---- argument validation ------------------------------------------------------------------------------------------------------
BASE = 0x7F0000000000        # stand-ins for device pointers: the check never looks behind them


def _gemm_args(**kw):
    M, N, K = 256, 64, 96
    live = np.array([1, 5, 2], np.int32)
    a = debug.DebugGemm()
    a.A, a.a_elems, a.lda = BASE, M * 104, 104
    a.Bt, a.bt_elems, a.ldb = BASE + (1 << 30), N * 96, 96
    a.M, a.N, a.K = M, N, K
    a.bias, a.bias_elems, a.n_real = BASE + (2 << 30), 61, 61
    a.relu = 1
    a.mask_out, a.mask_in, a.mask_bytes, a.mask_cols = BASE + (3 << 30), None, (M // 32) * 9 * 32, 9
    a.Cb, a.cb_elems, a.ldc, a.c_col0 = BASE + (4 << 30), M * 88, 88, 16
    a.Cf, a.cf_elems, a.ldcf = None, 0, 0
    a.live, a.n_live, a.live_dev, a.live_dev_elems = live.ctypes.data, 3, BASE + (5 << 30), 4
    a._keep = live
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _wgrad_args(**kw):
    K, N, steps = 320, 224, 12
    live = np.array([1, 2, 5], np.int32)
    a = debug.DebugWgrad()
    a.X, a.x_elems, a.ldx = BASE, steps * 32 * 328, 328
    a.Z, a.z_elems, a.ldz = BASE + (1 << 30), steps * 32 * 224, 224
    a.steps, a.N, a.K = steps, N, K
    a.grad, a.grad_elems = BASE + (2 << 30), 263 * 200 + 200
    a.w_off, a.b_off, a.n_real = 0, 263 * 200, 200
    a.n_seg = 2
    for i, v in enumerate((0, 200, 0, 256, 63, 200)):
        a.seg[i] = v
    a.partial, a.partial_elems = BASE + (3 << 30), debug.wgrad_partial_floats(K, N)
    a.live, a.n_live, a.live_dev, a.live_dev_elems = live.ctypes.data, 3, BASE + (5 << 30), 4
    a.selector = 0
    a._keep = live
    for k, v in kw.items():
        if k == "seg":
            for i, x in enumerate(v):
                a.seg[i] = x
        else:
            setattr(a, k, v)
    return a


GEMM_BAD = [dict(M=0), dict(M=192), dict(M=-128), dict(N=0), dict(N=48), dict(K=0), dict(K=100), dict(A=None), dict(Bt=None),
            dict(A=BASE + 8), dict(Bt=BASE + 2), dict(lda=88), dict(lda=100), dict(ldb=95), dict(ldb=90), dict(a_elems=255 * 104 + 95),
            dict(bt_elems=63 * 96 + 95), dict(n_real=65), dict(n_real=-1), dict(bias_elems=60), dict(Cb=None),
            dict(Cf=BASE + (6 << 30), cf_elems=1 << 20, ldcf=64), dict(Cb=None, Cf=BASE + (6 << 30), cf_elems=256 * 64, ldcf=64),
            dict(ldc=87), dict(c_col0=15), dict(c_col0=-2), dict(c_col0=32), dict(cb_elems=255 * 88 + 16 + 63), dict(Cb=BASE + (4 << 30) + 2),
            dict(mask_cols=7), dict(mask_bytes=8 * 9 * 32 - 1), dict(mask_out=BASE + (3 << 30) + 4), dict(mask_in=BASE + (7 << 30)),
            dict(mask_out=None, mask_in=BASE + (7 << 30)),       # the dgrad form takes neither bias nor relu
            dict(n_live=9), dict(live_dev=None), dict(live_dev_elems=3), dict(live=None),
            dict(_list=[1, 8, 2]), dict(_list=[1, -1, 2])]
WGRAD_BAD = [dict(steps=0), dict(steps=-4), dict(N=0), dict(N=200), dict(K=0), dict(K=300), dict(X=None), dict(Z=None), dict(X=BASE + 4),
             dict(Z=BASE + 8), dict(ldx=312), dict(ldx=324), dict(ldz=216), dict(ldz=228), dict(ldz=220), dict(x_elems=383 * 328 + 319),
             dict(z_elems=383 * 224 + 223), dict(grad=None), dict(grad=BASE + 2), dict(n_real=0), dict(n_real=225), dict(w_off=-1), dict(b_off=-1),
             dict(n_seg=0), dict(n_seg=3), dict(seg=(0, 200, 0, 256, 65, 200)), dict(seg=(0, 200, 0, 199, 63, 200)), dict(seg=(-1, 200, 0, 256, 63, 200)),
             dict(seg=(0, 0, 0, 256, 63, 200)), dict(seg=(0, 200, 0, 256, 63, 201)), dict(b_off=263 * 200 - 1), dict(seg=(0, 200, -1, 256, 63, 200)), dict(w_off=1),
             dict(b_off=263 * 200 + 1), dict(grad_elems=263 * 200 + 199), dict(partial_elems=debug.wgrad_partial_floats(320, 224) - 1),
             dict(partial=BASE + 1), dict(selector=2),
             dict(n_live=13), dict(live_dev=None), dict(live_dev_elems=3), dict(live=None),
             dict(_list=[1, 12, 2]), dict(_list=[2, 1, 5]), dict(_list=[1, 1, 5])]        # deterministic mode: strictly ascending


@pytest.mark.parametrize("what,make,bad", [(0, _gemm_args, GEMM_BAD), (1, _wgrad_args, WGRAD_BAD)], ids=["gemm", "wgrad"])
def test_entry_points_refuse_bad_arguments_before_any_launch(what, make, bad):
    lib = debug.load()
    entry = lib.knerf_debug_generic_gemm if what == 0 else lib.knerf_debug_generic_wgrad
    assert lib.knerf_debug_generic_check(what, C.byref(make())) == 0                  # the base is fine: each change below is the reason
    assert lib.knerf_debug_generic_check(what, None) == _lib.KNERF_ERR_INVALID and entry(None, None) == _lib.KNERF_ERR_INVALID
    assert lib.knerf_debug_generic_check(2, C.byref(make())) == _lib.KNERF_ERR_INVALID
    for kw in bad:
        kw = dict(kw)
        lst = kw.pop("_list", None)
        a = make(**kw)
        if lst is not None:
            arr = np.array(lst, np.int32)
            a.live, a._keep = arr.ctypes.data, arr
        assert lib.knerf_debug_generic_check(what, C.byref(a)) == _lib.KNERF_ERR_INVALID, kw or lst
        # the entry point runs the same check first: it returns here, before any HIP call
        assert entry(None, C.byref(a)) == _lib.KNERF_ERR_INVALID, kw or lst
    if what == 1:       # an unordered list is fine without `partial` (atomic mode), the per-wave arena with its own size
        a = make(partial=None, partial_elems=0)
        arr = np.array([2, 1, 5], np.int32)
        a.live, a._keep = arr.ctypes.data, arr
        assert lib.knerf_debug_generic_check(1, C.byref(a)) == 0
        assert lib.knerf_debug_generic_check(1, C.byref(make(selector=1, partial_elems=debug.wgrad_partial_floats(320, 224, True)))) == 0
    else:               # the fp32 head form
        ok = make(Cb=None, cb_elems=0, Cf=BASE + (6 << 30), cf_elems=256 * 64, ldcf=64, relu=0, mask_out=None, mask_bytes=0)
        assert lib.knerf_debug_generic_check(0, C.byref(ok)) == 0
        ok.cf_elems -= 1
        assert lib.knerf_debug_generic_check(0, C.byref(ok)) == _lib.KNERF_ERR_INVALID


def test_python_wrappers_check_the_live_list_on_the_host():
    a = debug.DebugGemm()
    with pytest.raises(ValueError):
        debug._live_fields(a, [0, 4], 4, "cpu")
    with pytest.raises(ValueError):
        debug._live_fields(a, [-1], 4, "cpu")
    with pytest.raises(ValueError):
        debug._live_fields(a, [2, 1], 4, "cpu", ascending=True)
    assert debug._live_fields(a, None, 4, "cpu") is None and a.n_live == -1
    host, scratch = debug._live_fields(a, [2, 1], 4, "cpu")
    assert a.n_live == 2 and a.live_dev_elems == 3 and host.dtype == np.int32


def test_partial_arena_covers_every_grid():
    for K, N, steps, *_ in R.WGRAD_CASES:
        for pw in (False, True):
            d = debug.wgrad_launch(K, N, steps, per_wave=pw)
            assert d["gx"] * d["gy"] * d["units"] * d["slab_floats"] <= debug.wgrad_partial_floats(K, N, pw)
