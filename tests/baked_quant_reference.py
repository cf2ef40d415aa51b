"""NumPy restatement of the 8-bit brick codec (include/knerf.h knerf_baked_qbricks), written from the format text and independently of
the package's mirrors (keras_nerf_amd/baked_quant.py): arithmetic in float64 (every product of the format is exact there as well), the
exponent by exact comparison of 127 * 2.0 ** e against M over e = -24 .. 9, brick by brick and band by band."""
import numpy as np

E_MIN, E_MAX = -24, 9
RECORD_BYTES = {0: 16, 1: 32, 2: 64, 3: 112}
QRECORD_BYTES = {0: 8, 1: 16, 2: 32, 3: 64}


def band(k):
    """the SH band of coefficient k: the l with l^2 <= k < (l + 1)^2"""
    l = 0
    while (l + 1) * (l + 1) <= k:
        l += 1
    return l


def exponent(M):
    """the smallest integer e in [-24, 9] with 127 2^e >= M; 9 if there is none"""
    for e in range(E_MIN, E_MAX + 1):
        if 127.0 * 2.0 ** e >= M:
            return e
    return E_MAX


def coefficients(records, degree):
    """the stored fp16 coefficients of brick records uint8 [n, P, record bytes] as float64 [n, P, K, 3]"""
    K = (degree + 1) ** 2
    rec = np.asarray(records, dtype=np.uint8)
    assert rec.ndim == 3 and rec.shape[2] == RECORD_BYTES[degree]
    return np.ascontiguousarray(rec[:, :, 4:4 + 6 * K]).view("<f2").reshape(rec.shape[0], rec.shape[1], K, 3).astype(np.float64)


def quantize(records, degree):
    """brick records uint8 [n, P, record bytes] -> (quantised records uint8 [n, P, quantised record bytes], exponents uint32 [n])"""
    K = (degree + 1) ** 2
    rec = np.asarray(records, dtype=np.uint8)
    co = coefficients(rec, degree)
    n, P = rec.shape[:2]
    out = np.zeros((n, P, QRECORD_BYTES[degree]), dtype=np.uint8)
    words = np.zeros(n, dtype=np.uint32)
    out[:, :, 0:4] = rec[:, :, 0:4]
    for s in range(n):
        word = 0
        for l in range(degree + 1):
            ks = [k for k in range(K) if band(k) == l]
            c = co[s][:, ks, :]
            mag = np.abs(c)
            mag[np.isnan(c)] = 0.0
            e = exponent(float(mag.max()))
            word |= (e & 0xFF) << (8 * l)
            with np.errstate(invalid="ignore"):
                q = np.rint(c * 2.0 ** (-e))                               # rint: to nearest, ties to even
            q = np.minimum(np.maximum(q, -127.0), 127.0)
            q[np.isnan(c)] = 0.0
            q = q.astype(np.int64)
            for i, k in enumerate(ks):
                for ch in range(3):
                    out[s, :, 4 + 3 * k + ch] = (q[:, i, ch] & 0xFF).astype(np.uint8)
        words[s] = word
    return out, words


def exponents_of(words, degree):
    """int64 [n, degree + 1]: the used exponent bytes as signed numbers"""
    w = np.asarray(words, dtype=np.uint32).astype(np.int64)
    e = np.stack([(w >> (8 * l)) & 0xFF for l in range(degree + 1)], axis=-1)
    return np.where(e >= 128, e - 256, e)


def decoded(qrecords, words, degree):
    """the decoded coefficients q 2^e as float64 [n, P, K, 3]"""
    K = (degree + 1) ** 2
    qr = np.asarray(qrecords, dtype=np.uint8)
    assert qr.ndim == 3 and qr.shape[2] == QRECORD_BYTES[degree]
    q = qr[:, :, 4:4 + 3 * K].astype(np.int64)
    q = np.where(q >= 128, q - 256, q).reshape(qr.shape[0], qr.shape[1], K, 3).astype(np.float64)
    e = exponents_of(words, degree)
    scale = np.stack([2.0 ** e[:, band(k)].astype(np.float64) for k in range(K)], axis=-1)                   # [n, K]
    return q * scale[:, None, :, None]


def dequantize(qrecords, words, degree):
    """(quantised records, exponents) -> brick records uint8 [n, P, record bytes]: sigma's bytes, the decoded values as fp16, zero padding"""
    K = (degree + 1) ** 2
    qr = np.asarray(qrecords, dtype=np.uint8)
    dec = decoded(qr, words, degree)
    h = dec.astype("<f2")
    assert np.array_equal(h.astype(np.float64), dec)                       # every decoded value is exactly an fp16 number
    out = np.zeros((qr.shape[0], qr.shape[1], RECORD_BYTES[degree]), dtype=np.uint8)
    out[:, :, 0:4] = qr[:, :, 0:4]
    out[:, :, 4:4 + 6 * K] = h.reshape(qr.shape[0], qr.shape[1], 3 * K).view(np.uint8)
    return out


def scaled_lattice(sigma, co, b):
    """the test lattice of the quantisation tests: the coefficients of point (x, y, z) in band l multiplied by
    2^-(((x // b) 7 + (y // b) 3 + (z // b)) mod 5) (1, 1/2, 1/8, 1/32)[l], rounded to fp16; sigma unchanged"""
    R = sigma.shape
    K = co.shape[-2]
    x, y, z = np.meshgrid(*(np.arange(r) for r in R), indexing="ij")
    brick = 2.0 ** -(((x // b) * 7 + (y // b) * 3 + (z // b)) % 5).astype(np.float64)
    per_band = np.array([(1.0, 0.5, 0.125, 0.03125)[band(k)] for k in range(K)])
    out = co.astype(np.float64) * brick[..., None, None] * per_band[None, None, None, :, None]
    return sigma, out.astype(np.float16)
