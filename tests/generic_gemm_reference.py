"""NumPy float64 reference of the general-shape path's matmul launchers (csrc/generic.hip launch_gemm / launch_wgrad), the cases
of tests/test_gpu_generic_gemm.py and the mutants tests/test_generic_gemm_host.py proves those cases can see.

    C  = A . Bt^T (+ bias[col < n_real]) (relu) (* relu bit)                        over all 32-row tiles or a live list
    dW[row(k)][n] += sum_m X[m][k] dZ[m][n],  db[n] += sum_m dZ[m][n]   (n < n_real; row(k) from the segment map (col0, width, wrow0))

Relu bits: [32-row tile][feature / 8][32 bytes]; byte 16 hh + i holds row (i & 3) + 8 (i >> 2) + 4 hh of the tile, bit j feature
8 octet + j (csrc/generic.h GemmArgs).

Two input families.
EXACT: every operand a small integer in [-3, 3] stored as bf16, biases integers or halves, gradients prefilled with integers.  Every
product is an integer <= 9, every partial sum of a contraction over n terms is bounded by 9 n (+ bias / prefill) < 2^24, so every
fp32 partial sum in ANY order is exact and the bf16 output is the round-to-nearest-even of an exactly known number: all
comparisons are == on bits.  `assert_exact` checks the 2^24 condition for every case.
REAL: Gaussian operands rounded to bf16 with about 20 % exact zeros.  bf16 x bf16 products are exact in fp32; a sum of n such
products (and one bias / prefill) formed by n fp32 additions in any order, rounding to nearest or truncating, is within
n 2^-23 (sum |a_k b_k| + |bias|) of the exact sum (each addition errs by at most 2^-23 of its result, every partial result is
bounded by the sum of magnitudes; first order).  bf16 outputs add half a bf16 ulp at |ref| + bound.  One row of A holds a single
1.0, so its accumulators are weights exactly: one bias cancels such an accumulator to exactly 0, another (over a zero weight) makes
it the smallest positive normal bf16.  No input produces a subnormal result.
"""
import numpy as np

from oracle.nerf_oracle import round_bf16

SENT_C = 0x5A5B            # bf16 sentinel of untouched outputs (a finite value no case produces: 1.5e16)
SENT_MASK = 0xA5
NAN_BF16 = 0x7FC1
TINY = float(np.float32(2.0 ** -126))       # the smallest positive normal bf16


# ---- bf16 ------------------------------------------------------------------------------------------------------------------
def to_bits(x):
    """fp32-representable values -> bf16 bit patterns (uint16), round to nearest even"""
    return (round_bf16(np.asarray(x, np.float32)).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def from_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def half_ulp_bf16(x):
    """half a bf16 ulp (8 significand bits) in the binade of |x| (normal range)"""
    m, e = np.frexp(np.maximum(np.abs(x), TINY))          # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, e - 1 - 8)


# ---- relu bits -------------------------------------------------------------------------------------------------------------
def _byte_rows():
    i = np.arange(16)
    return np.concatenate([(i & 3) + 8 * (i >> 2), (i & 3) + 8 * (i >> 2) + 4])      # byte 16 hh + i -> row of the tile


def mask_pack(bits, mask_cols, fill=SENT_MASK, natural=False):
    """bool [M][N] -> uint8 [M / 32][mask_cols][32]; octets >= N / 8 keep `fill`.  natural: the MUTANT order, byte b = row b"""
    M, N = bits.shape
    rows = np.arange(32) if natural else _byte_rows()
    t = bits.reshape(M // 32, 32, N // 8, 8)[:, rows]                                  # [tile][byte][octet][bit]
    by = (t.astype(np.uint16) << np.arange(8, dtype=np.uint16)).sum(axis=3).astype(np.uint8)
    out = np.full((M // 32, mask_cols, 32), fill, np.uint8)
    out[:, :N // 8] = by.transpose(0, 2, 1)
    return out


def mask_unpack(mask, N):
    """uint8 [tiles][mask_cols][32] -> bool [tiles * 32][N]"""
    T = mask.shape[0]
    by = mask[:, :N // 8].transpose(0, 2, 1)                                           # [tile][byte][octet]
    bits = ((by[..., None] >> np.arange(8, dtype=np.uint8)) & 1).astype(bool)          # [tile][byte][octet][bit]
    out = np.empty((T, 32, N // 8, 8), bool)
    out[:, _byte_rows()] = bits
    return out.reshape(T * 32, N)


# ---- cases -----------------------------------------------------------------------------------------------------------------
# (K, N, M, class the launch must reach: kernel, NT, gy, tiles per wave)
GEMM_CASES = [
    (32, 32, 128, ("ws", 1, 1, 1)),
    (64, 96, 128, ("ws", 1, 3, 1)),
    (96, 64, 384, ("ws", 2, 1, 1)),
    (160, 128, 384, ("ws", 4, 1, 1)),
    (256, 256, 384, ("ws", 8, 1, 1)),
    (320, 256, 384, ("ws", 4, 2, 1)),
    (288, 32, 384, ("ws", 1, 1, 1)),
    (32, 256, 131200, ("ws", 8, 1, 2)),
    (32, 512, 65664, ("ws", 8, 2, 2)),
    (608, 512, 16512, ("ws", 2, 8, 2)),
    # classes the coverage closure found in the suite's contexts and no row above reaches (tests/test_generic_gemm_host.py)
    (64, 512, 384, ("ws", 8, 2, 1)),            # deep_wide's first layer
    (64, 96, 43136, ("ws", 1, 3, 2)),           # odd_units' fine pass: gy = 3, second iteration
    (32, 384, 43136, ("ws", 4, 3, 2)),          # deep_wide's 512 x 512 layers are ws<4>, gy > 1, second iteration: the same at gy = 3
    (2400, 32, 384, ("stream", 1, 1, 1)),
    (2400, 64, 384, ("stream", 2, 1, 1)),
    (2400, 128, 384, ("stream", 4, 1, 1)),
    (2400, 256, 384, ("stream", 8, 1, 1)),
]
LARGE_M = 4096             # rows above this: exact family only, no fp32 output
# (K, N, steps, segments, n_real, class: gx, gy, gz, shortest and longest schedule of a unit)
WGRAD_CASES = [
    (32, 32, 4, ((0, 32, 0),), 4, (1, 1, 4, 1, 1)),
    (96, 160, 12, ((0, 96, 0),), 157, (1, 1, 12, 1, 1)),
    (256, 256, 300, ((0, 256, 0),), 256, (1, 1, 256, 1, 2)),
    (64, 32, 1300, ((0, 63, 0),), 30, (1, 1, 256, 5, 6)),
    (320, 256, 4, ((0, 256, 0), (256, 63, 256)), 256, (2, 1, 8, 0, 1)),
    (320, 256, 100, ((0, 256, 0), (256, 63, 256)), 256, (2, 1, 96, 1, 2)),
    (608, 512, 100, ((0, 512, 0), (512, 63, 512)), 512, (3, 2, 40, 2, 3)),
    (320, 224, 12, ((0, 200, 0), (256, 63, 200)), 200, (2, 1, 8, 1, 2)),
    # found by the coverage closure: more than one block AND a ring that wraps, as deep_wide's 512 x 512 layers have
    (320, 256, 700, ((0, 256, 0), (256, 63, 256)), 256, (2, 1, 128, 5, 6)),
]
PER_WAVE_ROWS = (0, 1, 2, 7)       # the per-wave wgrad_kernel (selector 1) also runs on the first three rows and the two-segment row


def gemm_class(d):
    """(kernel, NT, gy, tiles per wave capped at 2) of a debug.gemm_launch() description"""
    return (d["kernel"], d["nt"], d["gy"], min(d["tiles_per_wave"], 2))


def unit_counts(steps, units, deterministic, live=None):
    """schedule length of every accumulating unit (csrc/generic.hip unit_schedule)"""
    n = steps if live is None else len(live)
    if not deterministic:
        return [(n - u + units - 1) // units if n > u else 0 for u in range(units)]
    if live is None:
        return [(u + 1) * steps // units - u * steps // units for u in range(units)]
    lv = np.asarray(live)
    return [int(np.searchsorted(lv, (u + 1) * steps // units) - np.searchsorted(lv, u * steps // units)) for u in range(units)]


def wgrad_class(d, steps):
    """(kernel, gx gy > 1, idle units, schedule-length classes present) of a debug.wgrad_launch() description; a schedule is short
    (< 3: shorter than the DMA ring's look-ahead), 3..4, or long (> 4: the four-buffer ring wraps)"""
    cls = set()
    for det in (False, True):
        for c in unit_counts(steps, d["units"], det):
            if c:
                cls.add("short" if c < 3 else ("mid" if c <= 4 else "long"))
    idle = steps < d["units"]
    return (d["kernel"], d["gx"] * d["gy"] > 1, idle, tuple(sorted(cls)))


def live_lists(tiles, rng):
    """the live-tile lists of a case: None (no list), empty, one tile, a random third ascending, the same third shuffled, and (for the
    GEMMs) all but two tiles in random order"""
    third = np.sort(rng.choice(tiles, size=max(1, tiles // 3), replace=False)).astype(np.int32)
    shuf = third.copy()
    if len(shuf) > 1:
        while np.array_equal(shuf, third):
            rng.shuffle(shuf)
    most = rng.permutation(tiles)[:max(tiles - 2, 1)].astype(np.int32)      # longer than one pass of a persistent grid: later iterations walk the list too
    return {"none": None, "empty": np.zeros(0, np.int32), "one": np.array([tiles * 2 // 3], np.int32), "third": third, "shuffled": shuf,
            "most": most}


def _values(rng, shape, family):
    """operand values (float32, exactly bf16)"""
    if family == "exact":
        return rng.integers(-3, 4, size=shape).astype(np.float32)
    v = round_bf16(rng.standard_normal(shape).astype(np.float32))
    v[rng.random(shape) < 0.2] = 0.0
    return v


def gemm_inputs(K, N, M, family, seed=0):
    """One GEMM case's operands, shared by every mode.  Leading dimensions are wider than the operands and the pad holds bf16 NaN:
    nothing may read it.  A, Bt: float32 values [M][K], [N][K]; bias [N] (non-zero also at columns >= n_real, where it must not
    be applied); n_real; mask_bits [M][N]: the reference-built relu bits of the dgrad mode."""
    rng = np.random.default_rng([seed, K, N, M, family == "exact"])
    A, Bt = _values(rng, (M, K), family), _values(rng, (N, K), family)
    n_real = 4 if N == 32 else N - 3
    if family == "exact":
        bias = (rng.integers(-9, 10, size=N) * 0.5).astype(np.float32)
        bias[bias == 0] = 0.5
    else:
        bias = rng.standard_normal(N).astype(np.float32)
        # row 5 of A: a single 1.0 at column 3 -> its accumulators are Bt[:, 3] exactly; column 0: cancelled to exactly 0,
        # column 1: a zero weight and the smallest positive normal bf16 as bias
        A[5] = 0.0
        A[5, 3] = 1.0
        Bt[0, 3] = 1.25
        bias[0] = -1.25
        Bt[1, 3] = 0.0
        bias[1] = TINY
    return dict(K=K, N=N, M=M, family=family, A=A, Bt=Bt, bias=bias, n_real=n_real, mask_bits=rng.random((M, N)) < 0.6,
                lda=K + 8, ldb=K + 16, ldc=N + 24, c_col0=16, ldcf=N + 3, mask_cols=N // 8 + 1, lists=live_lists(M // 32, rng))


def padded_bits(V, ld, pad=NAN_BF16, extra_rows=0):
    """float32 values [rows][cols] -> uint16 [rows + extra_rows][ld] with `pad` everywhere else"""
    out = np.full((V.shape[0] + extra_rows, ld), pad, np.uint16)
    out[:V.shape[0], :V.shape[1]] = to_bits(V)
    return out


def wgrad_inputs(K, N, steps, segs, n_real, family, seed=0):
    """One weight-gradient case.  X [M][K], Z [M][N] hold non-zero data in EVERY column, also in the padding columns of X between and
    behind the segments and in the columns of Z at and above n_real: it must land nowhere.  The gradient is a flat buffer with
    guard elements in front of, between and behind the kernel and the bias: [7 guard][kernel rows x n_real][5 guard][n_real][9 guard]
    (head form, n_real = 4: kernel at 0 and the bias right behind it at 4 K, as the aux buffer has them)."""
    rng = np.random.default_rng([seed, K, N, steps, family == "exact", 1])
    M = steps * 32
    X, Z = _values(rng, (M, K), family), _values(rng, (M, N), family)
    if family == "exact":           # no all-zero tails: every padding column and padded feature column carries data
        X[X == 0] = 1.0
        Z[:, n_real:][Z[:, n_real:] == 0] = 2.0
    rows = max(r0 + w for _, w, r0 in segs)
    if n_real == 4:
        w_off, b_off = 0, 4 * K
        n_grad = 4 * K + 4 + 9
    else:
        w_off, b_off = 7, 7 + rows * n_real + 5
        n_grad = b_off + n_real + 9
    if family == "exact":
        grad0 = rng.integers(-5, 6, size=n_grad).astype(np.float32)
        grad0[grad0 == 0] = 3.0
    else:
        grad0 = (64.0 * rng.standard_normal(n_grad)).astype(np.float32)      # large against the bound of the longest contraction: += must show
    return dict(K=K, N=N, steps=steps, M=M, family=family, X=X, Z=Z, segs=segs, n_real=n_real, w_off=w_off, b_off=b_off, grad0=grad0,
                kernel_rows=rows, ldx=K + 8, ldz=N + 16, lists=live_lists(steps, rng))


def assert_exact(n_terms, extra=0.0):
    """the exact family's condition: every partial sum of n_terms products of magnitude <= 9 (+ extra) stays below 2^24"""
    assert 9 * n_terms + extra < 2 ** 24, (n_terms, extra)


# ---- references ------------------------------------------------------------------------------------------------------------
def _live_rows(M, live, rows=None):
    """bool [M]: rows of processed tiles (within the row window `rows`, a slice, if given)"""
    m = np.ones(M // 32, bool) if live is None else np.isin(np.arange(M // 32), live)
    m = np.repeat(m, 32)
    return m if rows is None else m[rows]


def gemm_reference(c, mode, live=None, mask_bits=None, rows=None, nt=1, mutant=None, victim=None):
    """float64 reference of one launch on case c (gemm_inputs).  mode: "forward" (bias, relu, bits out), "norelu" (bias),
    "head" (bias, fp32 out), "dgrad" (no bias; * mask_bits).  rows: a slice of rows to evaluate (rows are independent).
    Returns dict(value [R][N] float64 -- the exact result before the output rounding --, bound [R][N]: n 2^-23 sum |a b| (+ |bias|)
    (real-valued family; None in the exact one),
    touched bool [R]: rows the launch writes, bits bool [R][N] or None: relu bits of the forward mode, decided on the bf16-ROUNDED
    value).  mutant: one of GEMM_MUTANTS; victim: the tile the skip mutant drops."""
    K, N, M = c["K"], c["N"], c["M"]
    sl = slice(0, M) if rows is None else rows
    A = c["A"][sl].astype(np.float64)
    Bt = c["Bt"].astype(np.float64)
    touched = _live_rows(M, live, sl)
    if mutant == "skip_tile":
        t = np.arange(M // 32)[:, None].repeat(32, 1).reshape(-1)[sl]
        touched = touched & (t != victim)
    Ke = K // 64 * 64 if mutant == "k_tail" else K
    real = c["family"] != "exact"                           # the magnitudes feed the real-valued family's bound only
    key = ("_products", sl.start, sl.stop, Ke)              # the two products of a case are formed once and shared by its launches
    if key not in c:
        acc = A[:, :Ke] @ Bt[:, :Ke].T
        c[key] = (acc, np.abs(A[:, :Ke]) @ np.abs(Bt[:, :Ke]).T if real else None)
    acc, mag = c[key]
    if not touched.all():                                   # dead rows hold NaN on the device and are not read
        dead = ~touched[:, None]
        acc, mag = np.where(dead, 0.0, acc), np.where(dead, 0.0, mag) if real else None
    if mutant == "col_assign" and nt > 1:                   # accumulator t of lane r stored at n0 + 32 t + r, holding n0 + NT r + t
        nb = 32 * nt
        src = np.arange(N)
        j = src % nb
        src = src - j + nt * (j % 32) + j // 32
        acc, mag = acc[:, src], mag[:, src] if real else None
    bits = None
    if mode == "dgrad":
        mb = mask_bits[sl]
        if mutant == "mask_natural":
            mb = mask_unpack(mask_pack(mask_bits, N // 8, natural=True), N)[sl]
        acc = np.where(mb, acc, 0.0)
    else:
        b = c["bias"].astype(np.float64).copy()
        if mutant != "bias_pad":
            b[c["n_real"]:] = 0.0
        acc = acc + b
        mag = mag + np.abs(b) if real else None
        if mode == "forward":
            acc = np.maximum(acc, 0.0)
            # the bit is what a reader of the STORED bf16 value would decide; the mutant decides on the unrounded value
            bits = acc > 0 if mutant == "bit_pre_round" else from_bits(to_bits(acc.astype(np.float32))) > 0
    if c["family"] == "exact":
        assert_exact(K, 4.5)
        assert np.all(np.abs(acc) < 2 ** 24)
    return dict(value=acc, bound=K * 2.0 ** -23 * mag if real else None, touched=touched, bits=bits)


GEMM_MUTANTS = ("col_assign", "k_tail", "skip_tile", "bias_pad", "bit_pre_round", "mask_natural")


def expected_cb(ref, prior=SENT_C):
    """bf16 bit patterns [R][N] of an exact-family bf16 output: RNE of the exact value on touched rows, `prior` elsewhere"""
    out = to_bits(ref["value"].astype(np.float32))
    out[out == 0x8000] = 0                                  # an exact zero sum is +0 on the device as well (no negative zero arises
    return np.where(ref["touched"][:, None], out, np.uint16(prior))      # from x + 0.0 or max(x, 0))


def seg_row(segs, K, mutant=None):
    """kernel row of every buffer column k, or -1 (padding)"""
    row = np.full(K, -1)
    for c0, w, r0 in segs:
        row[c0:c0 + w] = r0 + np.arange(w)
    if mutant == "seg_pad" and len(segs) == 2:              # the padding behind segment 0 continues its kernel rows
        (c0, w, r0), c1 = segs[0], segs[1][0]
        row[c0 + w:c1] = r0 + w + np.arange(c1 - c0 - w)
    return row


def wgrad_reference(c, live=None, gx=1, mutant=None, victim=None):
    """float64 reference of one weight-gradient launch on case c (wgrad_inputs): dict(grad [n_grad] float64, bound [n_grad]).
    live: the list of steps to contract over (entries count as often as they appear).  gx: row blocks of the launch (the bias-block
    mutant).  mutant: one of WGRAD_MUTANTS; victim: the step the skip / double mutants pick."""
    K, N, steps, n_real = c["K"], c["N"], c["steps"], c["n_real"]
    lst = np.arange(steps) if live is None else np.asarray(live, np.int64)
    if mutant == "skip_tile":
        lst = lst[lst != victim]
    if mutant == "dup_tile":
        lst = np.concatenate([lst, [victim]])
    idx = (lst[:, None] * 32 + np.arange(32)).reshape(-1)
    X, Z = c["X"][idx].astype(np.float64), c["Z"][idx].astype(np.float64)
    dW, mW = X.T @ Z, np.abs(X).T @ np.abs(Z)
    db, mb = Z.sum(0), np.abs(Z).sum(0)
    if mutant == "bias_block":                              # every row block adds its column sums, not only bx == 0
        db, mb = db * gx, mb * gx
    g0 = c["grad0"].astype(np.float64)
    grad = np.zeros_like(g0) if mutant == "assign" else g0.copy()
    mag = np.abs(grad)
    written = np.zeros(len(g0), bool)
    row = seg_row(c["segs"], K, mutant)
    for k in np.nonzero(row >= 0)[0]:
        o = c["w_off"] + row[k] * n_real
        grad[o:o + n_real] += dW[k, :n_real]
        mag[o:o + n_real] += mW[k, :n_real]
        written[o:o + n_real] = True
    o = c["b_off"]
    grad[o:o + n_real] += db[:n_real]
    mag[o:o + n_real] += mb[:n_real]
    written[o:o + n_real] = True
    if mutant == "assign":
        grad = np.where(written, grad, g0)
    if c["family"] == "exact":
        assert_exact(max(len(idx), 1) * max(gx, 1), 5.0)
        assert np.all(np.abs(grad) < 2 ** 24)
    return dict(grad=grad, bound=max(len(idx), 1) * 2.0 ** -23 * mag, written=written)


WGRAD_MUTANTS = ("skip_tile", "dup_tile", "seg_pad", "bias_block", "assign")
