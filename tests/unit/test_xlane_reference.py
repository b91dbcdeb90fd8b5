"""The host referee of the cross-lane diagnostic (bgc_diag_xlane_expected: xlane_ref.h's model) against a model
written here in numpy from gpu_diag.h's text alone ("Cross-lane" in "the data the diagnostics generate").

The device is compared bit for bit with that referee (tests/gpu/test_diag_xlane.py), so the referee has to be
right on its own account, and it runs without a GPU.  The model here names every DPP control by its words and
works on index arrays; it shares no table and no decoding with xlane_ref.h.

* every result word and every digest, for three seeds and 1, 2 and 64 rounds;
* every word that is a pure permutation of its input is one;
* lane 63 of the prefix scan holds the sum of the wave;
* the lanes that the EXEC mask disables hold `old`, and the mask has lanes on and off.

model_round() is also what the GPU test holds the device's own words to."""
import numpy as np
import pytest

SEEDS = [0x5EED, 0, 0xFFFFFFFF]
ROUNDS = [1, 2, 64]
ROW, WAVE, MASK, ALU, SWAP, LDS, LANE, EXEC = range(8)
WORDS = (12, 6, 6, 3, 4, 6, 6, 4)
BASE = tuple(int(b) for b in np.cumsum((0,) + WORDS[:-1]))
L = np.arange(64)
ALL = np.ones(64, dtype=bool)
U32 = np.uint32


def mix32(x):
    x = np.array(x, dtype=np.uint32)
    x ^= x >> U32(16)
    x *= U32(0x7FEB352D)
    x ^= x >> U32(15)
    x *= U32(0x846CA68B)
    x ^= x >> U32(16)
    return x


def w(seed, cls, r, k):
    """operand word k of (class, round) for the 64 lanes"""
    return mix32(U32(seed) ^ mix32(U32(cls << 24 | r << 16 | k << 8) | L.astype(np.uint32)))


def u(seed, cls, r, k):
    """the wave-uniform word: the hash of lane 64"""
    return int(mix32(U32(seed) ^ mix32(U32(cls << 24 | r << 16 | k << 8 | 64))))


def source(ctrl, n=None):
    """(source lane of every lane, whether it is valid) for a DPP control named as the assembler names it"""
    row, i = L // 16 * 16, L % 16
    if ctrl == "quad_perm":
        return L // 4 * 4 + np.array(n)[L % 4], ALL
    if ctrl == "row_shl":
        return L + n, i + n < 16
    if ctrl == "row_shr":
        return L - n, i - n >= 0
    if ctrl == "row_ror":
        return row + (i - n) % 16, ALL
    if ctrl == "wave_shl":
        return L + 1, L < 63
    if ctrl == "wave_rol":
        return (L + 1) % 64, ALL
    if ctrl == "wave_shr":
        return L - 1, L > 0
    if ctrl == "wave_ror":
        return (L - 1) % 64, ALL
    if ctrl == "row_mirror":
        return row + 15 - i, ALL
    if ctrl == "row_half_mirror":
        return L // 8 * 8 + 7 - L % 8, ALL
    if ctrl == "row_bcast" and n == 15:  # row 0 reads itself
        return np.where(L >= 16, row - 1, L), ALL
    if ctrl == "row_bcast" and n == 31:  # rows 0 and 1 read themselves
        return np.where(L >= 32, 31, L), ALL
    raise ValueError(ctrl)


def dpp(vdst, src0, ctrl, n=None, row_mask=0xF, bank_mask=0xF, bound_ctrl=0, exec_=ALL, op=None, src1=None):
    """vdst after v_mov_b32_dpp (op None) or a VOP2 with a DPP first operand: the gate of gpu_diag.h"""
    s, valid = source(ctrl, n)
    s = np.where(valid, s, 0)
    written = exec_ & (((row_mask >> (L // 16)) & 1) == 1) & (((bank_mask >> (L % 16 // 4)) & 1) == 1)
    readable = valid & exec_[s]
    moved = np.where(readable, src0[s], U32(0))
    result = moved if op is None else op(moved, src1)
    return np.where(written & (readable | bool(bound_ctrl)), result, vdst).astype(np.uint32)


def add(a, b):
    return (a.astype(np.uint64) + b.astype(np.uint64)).astype(np.uint32)


def swap(width, vdst, src):
    """both results of v_permlane{width}_swap_b32"""
    upper = (L // width) % 2 == 1
    return np.where(upper, src[(L - width) % 64], vdst), np.where(~upper, vdst[(L + width) % 64], src)


def bpermute(addr, src, old=None, exec_=ALL):
    s = (addr >> U32(2)).astype(np.int64) & 63
    got = np.where(exec_[s], src[s], U32(0))
    return got if old is None else np.where(exec_, got, old)


def permute(addr, src):
    out = np.zeros(64, dtype=np.uint32)
    out[(addr >> U32(2)).astype(np.int64) & 63] = src
    return out


def swizzle(offset, src):
    if offset & 0x8000:
        return src[L // 4 * 4 + ((offset >> (2 * (L % 4))) & 3)]
    and_, or_, xor_ = offset & 31, (offset >> 5) & 31, (offset >> 10) & 31
    return src[L // 32 * 32 + (((L % 32) & and_ | or_) ^ xor_)]


def exec_mask(seed, r):
    on = u(seed, EXEC, r, 2) & 63
    off = (on + 1 + u(seed, EXEC, r, 3) % 63) & 63
    m = ((u(seed, EXEC, r, 1) << 32 | u(seed, EXEC, r, 0)) | 1 << on) & ~(1 << off)
    return np.array([(m >> l) & 1 for l in range(64)], dtype=bool)


ROW_STEPS = [("quad_perm", (3, 2, 1, 0)), ("quad_perm", (1, 0, 3, 2)), ("quad_perm", (2, 2, 0, 0)), ("row_shl", 1), ("row_shl", 7), ("row_shr", 1),
             ("row_shr", 12), ("row_ror", 1), ("row_ror", 8), ("row_ror", 15), ("row_mirror", None), ("row_half_mirror", None)]
WAVE_STEPS = [("wave_shl", 1), ("wave_rol", 1), ("wave_shr", 1), ("wave_ror", 1), ("row_bcast", 15), ("row_bcast", 31)]
MASK_STEPS = [("row_shr", 1, 0xF, 0xF, 1), ("wave_shl", 1, 0xF, 0xF, 1), ("row_ror", 3, 0xA, 0xF, 0), ("row_ror", 3, 0xF, 0x5, 0),
              ("row_bcast", 15, 0xA, 0xF, 0), ("row_shr", 3, 0x6, 0x9, 1)]


def model_round(seed, r):
    """the 47 result words of round r for the 64 lanes, [word, lane]"""
    out = []
    for cls, steps in ((ROW, ROW_STEPS), (WAVE, WAVE_STEPS), (MASK, MASK_STEPS)):
        src, old = w(seed, cls, r, 0), w(seed, cls, r, 1)
        out += [dpp(old, src, *step) for step in steps]
    a, b, c = (w(seed, ALU, r, k) for k in range(3))
    out.append(dpp(c, a, "row_shr", 1, bound_ctrl=1, op=add, src1=b))
    out.append(dpp(c, a, "row_ror", 8, op=np.minimum, src1=b))
    acc = dpp(c, c, "row_shr", 1, bound_ctrl=1, op=add, src1=c)
    acc = dpp(acc, c, "row_shr", 2, bound_ctrl=1, op=add, src1=acc)
    acc = dpp(acc, c, "row_shr", 3, bound_ctrl=1, op=add, src1=acc)
    acc = dpp(acc, acc, "row_shr", 4, bank_mask=0xE, op=add, src1=acc)
    acc = dpp(acc, acc, "row_shr", 8, bank_mask=0xC, op=add, src1=acc)
    acc = dpp(acc, acc, "row_bcast", 15, row_mask=0xA, op=add, src1=acc)
    acc = dpp(acc, acc, "row_bcast", 31, row_mask=0xC, op=add, src1=acc)
    out.append(acc)
    x, y = w(seed, SWAP, r, 0), w(seed, SWAP, r, 1)
    out += [*swap(16, x, y), *swap(32, x, y)]
    src = w(seed, LDS, r, 0)
    lanes = L.astype(np.uint32)
    out.append(bpermute((w(seed, LDS, r, 1) & U32(63)) << U32(2), src))
    out.append(bpermute(((lanes + U32(1 + u(seed, LDS, r, 0) % 63)) & U32(63)) << U32(2), src))
    out.append(permute(((U32(u(seed, LDS, r, 1) | 1) * lanes + U32(u(seed, LDS, r, 2))) & U32(63)) << U32(2), src))
    out += [swizzle(0x1B | 0x04 << 5 | 0x11 << 10, src), swizzle(0x0F | 0x10 << 5 | 0x0A << 10, src), swizzle(0x8000 | 1 | 3 << 2 | 0 << 4 | 2 << 6, src)]
    a, b, c = (w(seed, LANE, r, k) for k in range(3))
    ballot = (a & U32(1)).astype(bool)
    written = c.copy()
    written[u(seed, LANE, r, 2) & 63] = u(seed, LANE, r, 1)
    bits = sum(1 << int(l) for l in L[ballot])
    out += [np.full(64, a[u(seed, LANE, r, 0) & 63]), np.full(64, b[0]), written, np.full(64, bits & 0xFFFFFFFF, dtype=np.uint32),
            np.full(64, bits >> 32, dtype=np.uint32), (np.cumsum(ballot) - ballot).astype(np.uint32)]
    src, old, m = w(seed, EXEC, r, 0), w(seed, EXEC, r, 1), exec_mask(seed, r)
    out.append(dpp(old, src, "wave_ror", 1, exec_=m))
    out.append(dpp(old, src, "wave_ror", 1, bound_ctrl=1, exec_=m))
    out.append(bpermute((w(seed, EXEC, r, 2) & U32(63)) << U32(2), src, old=old, exec_=m))
    out.append(np.full(64, src[np.argmax(m)]))
    return np.array(out, dtype=np.uint32)


def model_digests(raw):
    """[class, lane]: the fold of raw[round, word, lane]"""
    d = np.array([np.full(64, 0x9E3779B9 + c, dtype=np.uint32) for c in range(8)])
    for rnd in range(raw.shape[0]):
        for c in range(8):
            for word in range(WORDS[c]):
                d[c] = mix32(d[c] ^ raw[rnd, BASE[c] + word])
    return d


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def expected(ops):
    """computed once, shared and left unchanged"""
    return {(seed, rounds): ops.xlane_expected(rounds, seed=seed) for seed in SEEDS for rounds in ROUNDS}


@pytest.fixture(scope="module")
def model():
    return {seed: np.array([model_round(seed, r) for r in range(max(ROUNDS))]) for seed in SEEDS}


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("seed", SEEDS, ids=[f"{s:#x}" for s in SEEDS])
def test_every_word_and_digest_equals_the_numpy_model(expected, model, seed, rounds):
    e = expected[(seed, rounds)]
    assert e["cu_key"] == -1 and e["simd"] == -1 and e["rate_cu_key"] == [-1] * 4
    assert e["raw"].shape == (rounds, 47, 64) and e["digests"].shape == (8, 64)
    want = model[seed][:rounds]
    assert np.array_equal(e["raw"], want), np.argwhere(e["raw"] != want)[:6]
    assert np.array_equal(e["digests"], model_digests(want))


# (class, word) whose result is a permutation of the w_0 of its class
PERMUTATIONS = [(ROW, k) for k in (0, 1, 7, 8, 9, 10, 11)] + [(WAVE, 1), (WAVE, 3), (LDS, 1), (LDS, 2), (LDS, 5)]


@pytest.mark.parametrize("seed", SEEDS, ids=[f"{s:#x}" for s in SEEDS])
def test_pure_permutation_words_are_permutations(expected, seed):
    raw = expected[(seed, 64)]["raw"]
    for r in range(64):
        for cls, word in PERMUTATIONS:
            got = raw[r, BASE[cls] + word]
            assert np.array_equal(np.sort(got), np.sort(w(seed, cls, r, 0))), (r, cls, word)
            assert not np.array_equal(got, w(seed, cls, r, 0)), (r, cls, word)  # and it moves something
        both = np.sort(np.concatenate([w(seed, SWAP, r, 0), w(seed, SWAP, r, 1)]))
        for first in (0, 2):  # a swap keeps the 128 values of its two registers
            assert np.array_equal(np.sort(raw[r, BASE[SWAP] + first:BASE[SWAP] + first + 2].ravel()), both)


@pytest.mark.parametrize("seed", SEEDS, ids=[f"{s:#x}" for s in SEEDS])
def test_prefix_scan_ends_in_the_sum_of_the_wave(expected, seed):
    raw = expected[(seed, 64)]["raw"]
    for r in range(64):
        x = w(seed, ALU, r, 2).astype(np.uint64)
        assert int(raw[r, BASE[ALU] + 2, 63]) == int(x.sum()) & 0xFFFFFFFF
        assert np.array_equal(raw[r, BASE[ALU] + 2], (np.cumsum(x) & np.uint64(0xFFFFFFFF)).astype(np.uint32))


@pytest.mark.parametrize("seed", SEEDS, ids=[f"{s:#x}" for s in SEEDS])
def test_lanes_that_exec_disables_hold_old(expected, seed):
    raw = expected[(seed, 64)]["raw"]
    for r in range(64):
        m, old, src = exec_mask(seed, r), w(seed, EXEC, r, 1), w(seed, EXEC, r, 0)
        assert m.any() and not m.all()
        for word in range(3):
            assert np.array_equal(raw[r, BASE[EXEC] + word][~m], old[~m]), (r, word)
        assert (raw[r, BASE[EXEC] + 3] == src[np.argmax(m)]).all()
        # an enabled lane whose source lane is disabled: `old` without bound_ctrl, 0 with it
        blocked = m & ~m[(L - 1) % 64]
        assert np.array_equal(raw[r, BASE[EXEC]][blocked], old[blocked]) and not raw[r, BASE[EXEC] + 1][blocked].any()
