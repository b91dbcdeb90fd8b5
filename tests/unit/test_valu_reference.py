"""The host referee of the vector-ALU diagnostic (bgc_diag_valu_expected: valu_ref.h's HostAlu) against a
reference written here from gpu_diag.h's text alone ("Vector ALU" in "the data the diagnostics generate").

The device is compared bit for bit with that referee (tests/gpu/test_diag_valu.py), so the referee has to be
right on its own account, and it runs without a GPU:

* the integer class and the dots in numpy unsigned arithmetic;
* FMA, add and multiply in fp32, fp16 and fp64 by exact integer arithmetic on the decoded operands (Python
  integers: value = m * 2^e) and one rounding to nearest even, which is what IEEE 754 defines for all of
  them, the fused ones included;
* the conversions against numpy's and torch's CPU casts;
* the transcendental words, which the referee only uses for an error bound, within one unit in the last
  place of numpy's float64 functions rounded to fp32;
* every digest as the fold of the words before it;
* no operand and no expected result is a NaN, an infinity or a denormal."""
import numpy as np
import pytest
import torch

SEEDS = [0x5EED, 0, 1, 0xFFFFFFFF, 0x9E3779B9]
ROUNDS = [1, 8]
INT32, FP32, FP16, FP64, CVT, DOT, TRANS = range(7)
WORDS = (13, 6, 3, 6, 5, 2, 5)
BASE = (0, 13, 19, 22, 28, 33, 35)
LANES = np.arange(64, dtype=np.uint32)
F32_EMIN, F16_EMIN = -8, -4  # BGC_VALU_F32_EMIN, BGC_VALU_F16_EMIN
FORMATS = {"f16": (11, 5), "f32": (24, 8), "f64": (53, 11)}  # precision with the hidden bit, exponent bits


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def expected(ops):
    """computed once, shared and left unchanged"""
    return {(seed, rounds): ops.valu_expected(rounds, seed=seed) for seed in SEEDS for rounds in ROUNDS}


def mix32(x):
    x = np.array(x, dtype=np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def w(seed, cls, r, k):
    """operand word k of (class, round) for the 64 lanes"""
    return mix32(np.uint32(seed) ^ mix32(np.uint32(cls << 24 | r << 16 | k << 8) | LANES))


def f32_bits(h, emin=F32_EMIN, mask=15):
    return (h & np.uint32(0x807FFFFF)) | ((np.uint32(127 + emin) + ((h >> np.uint32(23)) & np.uint32(mask))) << np.uint32(23))


def f16_bits(h):
    h = h & np.uint32(0xFFFF)
    return (h & np.uint32(0x83FF)) | ((np.uint32(15 + F16_EMIN) + ((h >> np.uint32(10)) & np.uint32(7))) << np.uint32(10))


def f16x2_bits(h):
    return f16_bits(h) | (f16_bits(h >> np.uint32(16)) << np.uint32(16))


def f64_bits(hi, lo):
    field = np.uint64(1023 + F32_EMIN) + ((hi.astype(np.uint64) >> np.uint64(20)) & np.uint64(15))
    return ((hi & np.uint32(0x800FFFFF)).astype(np.uint64) << np.uint64(32)) | (field << np.uint64(52)) | lo.astype(np.uint64)


# ---------------------------------------------------------------------------------------------
# exact arithmetic: a number is (m, e), m a Python integer, value m * 2^e

def decode(bits, fmt):
    """(m, e) of a normal number or zero; anything else fails the test"""
    p, ebits = FORMATS[fmt]
    bits = int(bits)
    sign, field, frac = bits >> (p - 1 + ebits), (bits >> (p - 1)) & ((1 << ebits) - 1), bits & ((1 << (p - 1)) - 1)
    if field == 0 and frac == 0:
        return 0, 0
    assert 0 < field < (1 << ebits) - 1, f"{fmt} {bits:#x} is a denormal, an infinity or a NaN"
    m = (1 << (p - 1)) | frac
    return (-m if sign else m), field - ((1 << (ebits - 1)) - 1) - (p - 1)


def encode(m, e, fmt):
    """m * 2^e rounded once to nearest even; the result must be a normal number or zero"""
    p, ebits = FORMATS[fmt]
    if m == 0:
        return 0  # an exact cancellation is +0 in round-to-nearest
    sign, m = int(m < 0), abs(m)
    n = m.bit_length()
    if n > p:
        shift = n - p
        q, rem, half = m >> shift, m & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
        if q.bit_length() > p:
            q >>= 1
            shift += 1
        m, e = q, e + shift
    else:
        m, e = m << (p - n), e - (p - n)
    field = e + (p - 1) + ((1 << (ebits - 1)) - 1)
    assert 0 < field < (1 << ebits) - 1, f"{fmt} result with exponent field {field}: not a normal number"
    return sign << (p - 1 + ebits) | field << (p - 1) | (m & ((1 << (p - 1)) - 1))


def add(x, y):
    (mx, ex), (my, ey) = x, y
    e = min(ex, ey)
    return (mx << (ex - e)) + (my << (ey - e)), e


def mul(x, y):
    return x[0] * y[0], x[1] + y[1]


def neg(x):
    return -x[0], x[1]


def lanes(f, fmt, *operands):
    """f on the decoded operands lane by lane, encoded"""
    dtype = np.uint64 if fmt == "f64" else np.uint32
    return np.array([encode(*f(*(decode(o[i], fmt) for o in operands)), fmt) for i in range(64)], dtype=dtype)


def halves(f, *operands):
    lo = lanes(f, "f16", *(o & np.uint32(0xFFFF) for o in operands))
    hi = lanes(f, "f16", *(o >> np.uint32(16) for o in operands))
    return lo | (hi << np.uint32(16))


def fma(a, b, c):
    return add(mul(a, b), c)


# ---------------------------------------------------------------------------------------------
# the reference: the words of one round, [word][lane]

def ref_int32(seed, r):
    a, b, c = (w(seed, INT32, r, k) for k in range(3))
    a64, b64 = a.astype(np.uint64), b.astype(np.uint64)
    sh = c & np.uint32(31)
    ab = (a64 << np.uint64(32)) | b64
    sel = c & np.uint32(0x07070707)
    perm = np.zeros(64, dtype=np.uint32)
    for i in range(4):
        byte = (sel >> np.uint32(8 * i)) & np.uint32(7)
        perm |= ((ab >> (byte.astype(np.uint64) * np.uint64(8))) & np.uint64(0xFF)).astype(np.uint32) << np.uint32(8 * i)
    m24 = np.uint64(0xFFFFFF)
    return [a + b, a - b, a * b, ((a64 * b64) >> np.uint64(32)).astype(np.uint32),
            ((a64 & m24) * (b64 & m24)).astype(np.uint32) + c, a << sh, a >> sh, (a.view(np.int32) >> sh.astype(np.int32)).view(np.uint32),
            (a >> sh) & ((np.uint32(1) << ((c >> np.uint32(8)) & np.uint32(31))) - np.uint32(1)), perm,
            (ab >> sh.astype(np.uint64)).astype(np.uint32),
            np.array([bin(int(v)).count("1") for v in a], dtype=np.uint32),
            np.array([32 - int(v).bit_length() for v in a], dtype=np.uint32)]


def ref_fp32(seed, r):
    x = [f32_bits(w(seed, FP32, r, k)) for k in range(6)]
    p = lanes(mul, "f32", x[3], x[4])
    return [lanes(fma, "f32", x[0], x[1], x[2]), lanes(fma, "f32", x[3], x[5], x[1]), lanes(fma, "f32", x[4], x[0], x[2]), p,
            lanes(add, "f32", p, x[5]), lanes(lambda a, b: add(a, neg(b)), "f32", x[0], x[4])]


def fp16_operands(seed, r):
    a, b = f16x2_bits(w(seed, FP16, r, 0)), f16x2_bits(w(seed, FP16, r, 1))
    c = (f16x2_bits(w(seed, FP16, r, 2)) & np.uint32(0x7FFF7FFF)) | ((a ^ b) & np.uint32(0x80008000))
    return a, b, c


def ref_fp16(seed, r):
    a, b, c = fp16_operands(seed, r)
    return [halves(fma, a, b, c), halves(add, a, b), halves(mul, a, b)]


def fp64_operands(seed, r):
    return [f64_bits(w(seed, FP64, r, 2 * k), w(seed, FP64, r, 2 * k + 1)) for k in range(3)]


def ref_fp64(seed, r):
    x = fp64_operands(seed, r)
    out = []
    for v in (lanes(fma, "f64", *x), lanes(add, "f64", x[0], x[1]), lanes(mul, "f64", x[0], x[1])):
        out += [(v & np.uint64(0xFFFFFFFF)).astype(np.uint32), (v >> np.uint64(32)).astype(np.uint32)]
    return out


def ref_cvt(seed, r):
    x = [w(seed, CVT, r, k) for k in range(6)]
    f = [f32_bits(v).view(np.float32) for v in x]
    bf = torch.from_numpy(np.stack([f[4], f[5]])).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).astype(np.uint32)
    return [f[0].astype(np.int32).view(np.uint32), x[1].view(np.int32).astype(np.float32).view(np.uint32),
            f[2].astype(np.float16).view(np.uint16).astype(np.uint32),
            f16_bits(x[3]).astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32), bf[0] | (bf[1] << np.uint32(16))]


def ref_dot(seed, r):
    a, b, c = (w(seed, DOT, r, k) for k in range(3))
    sa, sb = a.view(np.int8).reshape(64, 4).astype(np.int64), b.view(np.int8).reshape(64, 4).astype(np.int64)
    ua, ub = a.view(np.uint8).reshape(64, 4).astype(np.int64), b.view(np.uint8).reshape(64, 4).astype(np.int64)
    signed = (sa * sb).sum(axis=1) + (c.view(np.int32) >> 8).astype(np.int64)
    unsigned = (ua * ub).sum(axis=1) + (c >> np.uint32(8)).astype(np.int64)
    return [(signed & 0xFFFFFFFF).astype(np.uint32), (unsigned & 0xFFFFFFFF).astype(np.uint32)]


def trans_operands(seed, r):
    x = [w(seed, TRANS, r, k) for k in range(5)]
    t = ((x[1] >> np.uint32(23)) & np.uint32(7)).astype(np.int64)
    log_in = (x[1] & np.uint32(0x007FFFFF)) | ((127 + np.where(t < 4, t - 5, t - 3)).astype(np.uint32) << np.uint32(23))
    pos = np.uint32(0x7FFFFFFF)
    return [f32_bits(x[0], -2, 7).view(np.float32), log_in.view(np.float32), f32_bits(x[2]).view(np.float32),
            (f32_bits(x[3]) & pos).view(np.float32), (f32_bits(x[4]) & pos).view(np.float32)]


def ref_trans(seed, r):
    x = [v.astype(np.float64) for v in trans_operands(seed, r)]
    return [np.exp2(x[0]), np.log2(x[1]), 1.0 / x[2], 1.0 / np.sqrt(x[3]), np.sqrt(x[4])]


EXACT = {INT32: ref_int32, FP32: ref_fp32, FP16: ref_fp16, FP64: ref_fp64, CVT: ref_cvt, DOT: ref_dot}


# ---------------------------------------------------------------------------------------------

def test_shape(expected):
    e = expected[(SEEDS[0], 8)]
    assert e["cu_key"] == -1 and e["simd"] == -1
    assert e["digests"].shape == (7, 64) and e["digests"].dtype == np.uint32
    assert e["raw"].shape == (8, 40, 64) and e["raw"].dtype == np.uint32
    assert sum(WORDS) == 40 and all(BASE[c] == sum(WORDS[:c]) for c in range(7))


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("seed", SEEDS, ids=[f"{s:#x}" for s in SEEDS])
@pytest.mark.parametrize("cls", EXACT, ids=["int32", "fp32", "fp16", "fp64", "cvt", "dot"])
def test_exact_class(expected, cls, seed, rounds):
    raw = expected[(seed, rounds)]["raw"]
    for r in range(rounds):
        ref = EXACT[cls](seed, r)
        assert len(ref) == WORDS[cls]
        for word, want in enumerate(ref):
            got = raw[r, BASE[cls] + word]
            assert np.array_equal(got, want), (r, word, np.flatnonzero(got != want)[:4], got[got != want][:4], want[got != want][:4])


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("seed", SEEDS, ids=[f"{s:#x}" for s in SEEDS])
def test_trans_words_are_libm_rounded_to_fp32(expected, seed, rounds):
    raw = expected[(seed, rounds)]["raw"]
    for r in range(rounds):
        for word, want in enumerate(ref_trans(seed, r)):
            got = raw[r, BASE[TRANS] + word].view(np.float32).astype(np.float64)
            ulp = np.exp2(np.floor(np.log2(np.abs(want))) - 23)
            assert np.all(np.abs(got - want) <= ulp), (r, word)


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("seed", SEEDS, ids=[f"{s:#x}" for s in SEEDS])
def test_digests_fold_the_words_in_order(expected, seed, rounds):
    e = expected[(seed, rounds)]
    for cls in range(7):
        d = np.full(64, 0x9E3779B9 + cls, dtype=np.uint32)
        for r in range(rounds):
            for word in range(WORDS[cls]):
                d = mix32(d ^ e["raw"][r, BASE[cls] + word])
        assert np.array_equal(e["digests"][cls], d), cls


def test_rounds_are_a_prefix_and_seeds_differ(expected):
    for seed in SEEDS:
        assert np.array_equal(expected[(seed, 8)]["raw"][:1], expected[(seed, 1)]["raw"])
    assert not np.array_equal(expected[(SEEDS[0], 8)]["digests"], expected[(SEEDS[1], 8)]["digests"])
    # per-lane operands: no two lanes of a class share a digest
    assert all(len(np.unique(expected[(SEEDS[0], 8)]["digests"][c])) == 64 for c in range(7))


def _normal_or_zero(bits, fmt):
    p, ebits = FORMATS[fmt]
    bits = bits.astype(np.uint64)
    field = (bits >> np.uint64(p - 1)) & np.uint64((1 << ebits) - 1)
    frac = bits & np.uint64((1 << (p - 1)) - 1)
    return np.all(((field > 0) & (field < (1 << ebits) - 1)) | ((field == 0) & (frac == 0)))


def _normal(bits, fmt):
    p, ebits = FORMATS[fmt]
    field = (bits.astype(np.uint64) >> np.uint64(p - 1)) & np.uint64((1 << ebits) - 1)
    return np.all((field > 0) & (field < (1 << ebits) - 1))


@pytest.mark.parametrize("seed", SEEDS, ids=[f"{s:#x}" for s in SEEDS])
def test_no_nan_infinity_or_denormal(expected, seed):
    """operands: normal numbers; results: normal numbers or an exact zero (a cancelled sum, i32 0 converted)"""
    raw = expected[(seed, 8)]["raw"]
    lo, hi = np.uint32(0xFFFF), np.uint32(16)
    for r in range(8):
        assert all(_normal(f32_bits(w(seed, FP32, r, k)), "f32") for k in range(6))
        assert all(_normal(h, "f16") for v in fp16_operands(seed, r) for h in (v & lo, v >> hi))
        assert all(_normal(v, "f64") for v in fp64_operands(seed, r))
        assert all(_normal(f32_bits(w(seed, CVT, r, k)), "f32") for k in (0, 2, 4, 5)) and _normal(f16_bits(w(seed, CVT, r, 3)), "f16")
        assert all(_normal(v.view(np.uint32), "f32") for v in trans_operands(seed, r))
        x = trans_operands(seed, r)
        assert np.all((x[1] <= 0.5) | (x[1] >= 2)) and np.all(x[1] > 0) and np.all(x[3] > 0) and np.all(x[4] > 0)
        assert all(_normal_or_zero(raw[r, BASE[FP32] + k], "f32") for k in range(6))
        assert all(_normal_or_zero(h, "f16") for k in range(3) for h in (raw[r, BASE[FP16] + k] & lo, raw[r, BASE[FP16] + k] >> hi))
        f64 = [raw[r, BASE[FP64] + 2 * k].astype(np.uint64) | (raw[r, BASE[FP64] + 2 * k + 1].astype(np.uint64) << np.uint64(32)) for k in range(3)]
        assert all(_normal_or_zero(v, "f64") for v in f64)
        assert _normal_or_zero(raw[r, BASE[CVT] + 1], "f32") and _normal(raw[r, BASE[CVT] + 2], "f16") and _normal(raw[r, BASE[CVT] + 3], "f32")
        bf = raw[r, BASE[CVT] + 4]
        assert _normal((bf & lo) << hi, "f32") and _normal(bf & np.uint32(0xFFFF0000), "f32")
        assert all(_normal(raw[r, BASE[TRANS] + k], "f32") for k in range(5))


def test_rounds_out_of_range_are_refused(ops):
    for rounds in (0, 65, -1):
        with pytest.raises(RuntimeError) as e:
            ops.valu_expected(rounds)
        assert str(e.value) == "valu diag: invalid arguments"
