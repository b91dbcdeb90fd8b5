"""The atomic check's host referee (native/gpu/hip/atomic_ref.h, through bgc_diag_atomic_expected and
bgc_diag_atomic_rate_expected) against an independent numpy model written from the text of gpu_diag.h, "Atomics": the
operands, the rows, the initial values and every class's final table for small launches; the referee's admissible
outcome of the cas and the tickets; the caps on an element's operations; the bounds that make the float sums exact in
any order, taken for the worst case (the sum of the magnitudes); and the rate phase's closed forms against a replay
of every iteration.  Needs no GPU: the referee touches no device."""
import numpy as np
import pytest

SEED = 0x5EED
EMPTY = 0xFFFFFFFF
CAPS = {"int32": 4096, "int64": 4096, "f32": 4096, "f64": 4096, "pk16": 128, "cas": 64, "ticket": 64}
CLASSES = ("int32", "int64", "f32", "f64", "pk16", "cas", "ticket", "lds")
GRIDS = [(4, 1), (4, 2), (4, 3), (9, 1), (9, 2), (9, 3)]
U32 = np.uint32


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


def _mix32(x):
    x = np.array(x, dtype=U32)
    x ^= x >> U32(16)
    x *= U32(0x7FEB352D)
    x ^= x >> U32(15)
    x *= U32(0x846CA68B)
    x ^= x >> U32(16)
    return x


class Launch:
    """every (wave, round, lane) of a launch, [wave, round, lane]"""

    def __init__(self, grid, rounds, seed=SEED):
        self.grid, self.rounds, self.seed = grid, rounds, seed
        self.w, self.r, self.l = np.meshgrid(np.arange(4 * grid), np.arange(rounds), np.arange(64), indexing="ij")
        self.pair = self.w * rounds + self.r
        self.pairs = 4 * grid * rounds
        self.id = (self.pair * 64 + self.l).astype(U32)

    def operand(self, cls, k):
        key = _mix32(U32(self.seed) ^ _mix32(U32(cls << 4 | k)))
        return _mix32(key ^ (self.w << 12 | self.r << 6 | self.l).astype(U32))

    def rows(self, placement, cls):
        """(row of every (wave, round, lane), rows of the table)"""
        if placement == "own":
            return 2 * (self.w // 4) + (self.w + self.r) % 2, 2 * self.grid
        n = -(-self.pairs // CAPS[cls])
        return self.pair % n, n


def _fold(ufunc, start, rows, row, lane, values, dtype=U32):
    table = np.full((rows, 64), start, dtype=dtype)
    ufunc.at(table, (row.ravel(), lane.ravel()), values.ravel().astype(dtype))
    return table


def _int_words(launch, cls, keys, row, rows):
    """add, smin, umax, and, or, xor of operand words keys[0..5], in that order"""
    a = [launch.operand(cls, k) for k in keys]
    return [_fold(np.add, 0, rows, row, launch.l, a[0]),
            _fold(np.minimum, 0x7FFFFFFF, rows, row, launch.l, a[1].view(np.int32), np.int32).view(U32),
            _fold(np.maximum, 0, rows, row, launch.l, a[2]),
            _fold(np.bitwise_and, 0xFFFFFFFF, rows, row, launch.l, a[3]),
            _fold(np.bitwise_or, 0, rows, row, launch.l, a[4]),
            _fold(np.bitwise_xor, 0, rows, row, launch.l, a[5])]


def _f32_values(h):
    return (h % U32(4095)).astype(np.int64) - 2047


def _trit(h):
    return (h % U32(3)).astype(np.int64) - 1


def _sum(launch, row, rows, values):
    return _fold(np.add, 0, rows, row, launch.l, values, np.int64)


def _cas_and_tickets(launch, row, rows, cap):
    """the lowest contender's id per element; the pullers per element; their id + 1 in ascending order; the lowest pair per row"""
    winner = _fold(np.minimum, EMPTY, rows, row, launch.l, launch.id)
    pullers = _sum(launch, row, rows, np.ones_like(row))
    order = np.zeros((rows, 64, cap), dtype=U32)
    for r in range(rows):
        ids = np.sort(launch.id[row == r].reshape(-1, 64), axis=0)  # every pair has all 64 lanes on one row
        order[r, :, :ids.shape[0]] = ids.T + 1
    first_pair = _fold(np.minimum, launch.pairs, rows, row, launch.l, launch.pair, np.int64)[:, 0]
    return winner, pullers, order, first_pair


@pytest.mark.parametrize("grid,rounds", GRIDS)
def test_the_referee_equals_the_numpy_model(ops, grid, rounds):
    e, launch = ops.atomic_expected(grid, rounds, seed=SEED), Launch(grid, rounds)
    layout = e["layout"]
    assert int(layout["pairs"]) == launch.pairs and int(layout["waves"]) == 4 * grid
    for pl, placement in enumerate(("own", "shared")):
        got = e[placement]
        for c, cls in enumerate(CLASSES[:7]):
            row, rows = launch.rows(placement, cls)
            assert int(layout["rows"][pl][c]) == rows, (placement, cls)
            count = _sum(launch, row, rows, np.ones_like(row))
            if placement == "shared":  # no element has more operations than its class's cap, and every row is used
                assert 1 <= count.min() and count.max() <= CAPS[cls], (cls, count.max())
            else:
                assert (count == 2 * rounds).all()
            if cls == "int32":
                for k, want in enumerate(_int_words(launch, 0, range(6), row, rows)):
                    assert np.array_equal(got[cls][k], want), (placement, cls, k)
            elif cls == "int64":
                a = launch.operand(1, 1).astype(np.uint64) << np.uint64(32) | launch.operand(1, 0).astype(np.uint64)
                assert np.array_equal(got[cls], _fold(np.add, 0, rows, row, launch.l, a, np.uint64)), placement
            elif cls == "f32":
                v = _f32_values(launch.operand(2, 0))
                assert np.abs(v).max() <= 2047 and _sum(launch, row, rows, np.abs(v)).max() < 2 ** 24  # exact in any order
                assert np.array_equal(got[cls][0], _sum(launch, row, rows, v).astype(np.float32).view(U32)), placement
            elif cls == "f64":
                v = (launch.operand(3, 0) >> U32(6)).astype(np.int64) - 2 ** 25
                assert np.abs(v).max() <= 2 ** 25 and _sum(launch, row, rows, np.abs(v)).max() < 2 ** 53
                assert np.array_equal(got[cls], _sum(launch, row, rows, v).astype(np.float64).view(np.uint64)), placement
            elif cls == "pk16":
                for k, (fmt, bits) in enumerate(((np.float32, 16), (np.float16, 0))):
                    h = launch.operand(4, k)
                    lo, hi = _trit(h), _trit(h >> U32(16))
                    assert _sum(launch, row, rows, np.abs(lo)).max() <= 128 and _sum(launch, row, rows, np.abs(hi)).max() <= 128

                    def half(values):
                        x = _sum(launch, row, rows, values).astype(fmt)
                        return (x.view(U32) >> U32(16)) if bits else x.view(np.uint16).astype(U32)

                    assert np.array_equal(got[cls][k], half(lo) | half(hi) << U32(16)), (placement, k)
            else:
                cap = int(layout["order_cap"][pl])
                assert cap == (2 * rounds if placement == "own" else -(-launch.pairs // rows))
                winner, pullers, order, first_pair = _cas_and_tickets(launch, row, rows, cap)
                assert pullers.max() <= cap
                if cls == "cas":
                    assert np.array_equal(got[cls][0], winner), placement
                    ballots = np.zeros(launch.pairs, dtype=np.uint64)
                    ballots[first_pair] = np.uint64(0xFFFFFFFFFFFFFFFF)
                    assert np.array_equal(e["ballots"][pl], ballots), placement
                else:
                    assert np.array_equal(got[cls][0], pullers.astype(U32)), placement
                    assert np.array_equal(e["order"][placement], order), placement
    # the LDS class: the OWN rows, words add, ticket, umax, smin, and, or, xor, add_f32, cas
    row, rows = launch.rows("own", "lds")
    lds = e["own"]["lds"]
    words = _int_words(launch, 7, (0, 3, 2, 4, 5, 6), row, rows)  # as add, smin, umax, and, or, xor
    for k, want in ((0, words[0]), (3, words[1]), (2, words[2]), (4, words[3]), (5, words[4]), (6, words[5])):
        assert np.array_equal(lds[k], want), k
    v = _f32_values(launch.operand(7, 7))
    assert _sum(launch, row, rows, np.abs(v)).max() < 2 ** 24
    assert np.array_equal(lds[7], _sum(launch, row, rows, v).astype(np.float32).view(U32))
    winner, pullers, order, first_pair = _cas_and_tickets(launch, row, rows, 2 * rounds)
    assert np.array_equal(lds[8], winner) and np.array_equal(lds[1], pullers.astype(U32))
    assert np.array_equal(e["order"]["lds"], order) and np.array_equal(e["ballots"][2], e["ballots"][0])
    assert int(layout["rows"][1][7]) == 0 and e["shared"]["lds"].size == 0
    assert (e["cu_keys"] == -1).all() and (e["rate_cu_keys"] == -1).all()


def test_the_caps_at_the_largest_launch():
    """2048 workgroups of 64 rounds: the rows of every SHARED class hold at most the class's cap of operations"""
    pairs = 4 * 2048 * 64
    for cls, cap in CAPS.items():
        rows = -(-pairs // cap)
        assert -(-pairs // rows) <= cap, cls
    assert 2047 * 4097 < 2 ** 24 and 2 ** 25 * 4097 < 2 ** 53 and 129 <= 256  # a doubled update stays exact as well


def test_a_plant_changes_the_referee_by_its_operand(ops):
    clean = ops.atomic_expected(4, 2, seed=SEED)
    launch = Launch(4, 2)
    a = launch.operand(0, 0)[5, 1, 9]
    row = int(launch.rows("own", "int32")[0][5, 1, 9])
    for times, delta in ((0, -int(a)), (2, int(a))):
        e = ops.atomic_expected(4, 2, plants=[("own", "int32", 0, 5, 1, 9, times, 0)], seed=SEED)
        diff = np.argwhere(e["words"] != clean["words"])
        assert diff.shape == (1, 1)
        assert int(e["own"]["int32"][0, row, 9]) == (int(clean["own"]["int32"][0, row, 9]) + delta) % 2 ** 32
    e = ops.atomic_expected(4, 2, plants=[("shared", "int32", 5, 5, 1, 9, 1, 0x10)], seed=SEED)
    row = int(launch.rows("shared", "int32")[0][5, 1, 9])
    assert int(e["shared"]["int32"][5, row, 9]) == int(clean["shared"]["int32"][5, row, 9]) ^ 0x10
    assert np.count_nonzero(e["words"] != clean["words"]) == 1


# ---------------------------------------------------------------------------------------------
# the rate phase

def _rate_replay(rate_grid, iters, cls, seed=SEED):
    """every iteration of every wave, one after the other: [group, row, lane] uint32, or the heads of rtn"""
    waves, groups = 4 * rate_grid, rate_grid // 8 * 4
    w, lane = np.meshgrid(np.arange(waves), np.arange(64), indexing="ij")
    group = (w // 4 // 8) * 4 + w % 4
    h = _mix32(_mix32(U32(seed) ^ _mix32(U32(0x100 | cls))) ^ (w << 6 | lane).astype(U32))
    if cls == 3:
        return np.bincount(group[:, 0], minlength=groups).astype(U32) * U32(iters)
    lo, hi, u = (np.zeros((groups, 64, 64), dtype=np.int64) for _ in range(3))
    worst = np.zeros((groups, 64, 64), dtype=np.int64)
    for i in range(iters):
        sign = -1 if (i // 64) % 2 else 1
        np.add.at(lo, (group, i % 64, lane), sign * _trit(h))
        np.add.at(hi, (group, i % 64, lane), sign * _trit(h >> U32(16)))
        np.add.at(u, (group, i % 64, lane), (h + U32((i * 0x9E3779B9) % 2 ** 32)).astype(np.int64))
        if i < 64:  # an adder's contribution to a word is 0 or its trit at any time: the worst partial sum is the adders' magnitudes
            np.add.at(worst, (group, i % 64, lane), np.abs(_trit(h)))
    assert worst.max() <= 8
    if cls == 0:
        return lo.astype(np.float32).view(U32)
    if cls == 1:
        return (lo.astype(np.float32).view(U32) >> U32(16)) | (hi.astype(np.float32).view(U32) >> U32(16)) << U32(16)
    return (u % 2 ** 32).astype(U32)


@pytest.mark.parametrize("iters", [1, 15, 16, 65])
@pytest.mark.parametrize("cls", range(4), ids=["f32", "pk_bf16", "u32", "rtn"])
def test_the_rate_closed_forms_equal_a_replay(ops, cls, iters):
    for rate_grid in (8, 24):
        got = ops.atomic_rate_expected(rate_grid, iters, cls, seed=SEED)
        want = _rate_replay(rate_grid, iters, cls)
        assert got.shape == want.shape and np.array_equal(got, want), (rate_grid, np.argwhere(got != want)[:4])
        if cls == 3:
            assert (got == 8 * iters).all()
        elif iters <= 64:
            assert not got[:, iters:].any()  # rows that no iteration visits stay 0
