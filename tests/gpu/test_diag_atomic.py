"""The atomic diagnostic (bgc_diag_atomic): every global and LDS atomic form in a table per workgroup (OWN) and in one
shared by the launch (SHARED), refereed by the host, and the four atomic rates.

* A clean run finds nothing, and the tables it leaves equal the host referee's word for word (the float classes as
  bits: every sum is exact in any order); every cas element has exactly one winner whose id it holds, and every order
  array is a permutation of its pullers' ids.  The referee is checked on its own against an independent model in
  tests/unit/test_atomic_reference.py.
* A lost update (times 0) and a doubled one (times 2) on one lane give exactly one wrong word, in the right table, row
  and lane, and its delta is the lane's operand, taken from the referee run with the same plant.  The operations that
  do not see a repeat (smin, umax, and, or, cas) take a wrong operand instead, chosen to dominate; the referee says
  whether it must show.  In SHARED the `and` and `or` words have seen 2048 hashed operands at these sizes and are
  saturated, so no single operand can show there: the test asserts that the referee says so and that the run is clean.
* For OWN and LDS the CU key that the result names equals the one the planted workgroup recorded in that same run.
* A rate plant clears rate_ok and nothing else; a wave made to wait 20 ms shows in its class's time and names its XCC.

Every plant changes how often one lane issues one atomic, or one operand; no kernel reads or writes out of bounds and
every one runs to completion.  No assertion compares with a measured rate."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED
SMALL = dict(wgs_per_cu=1, rounds=2, rate_iters=15)
ROUNDS = SMALL["rounds"]
NONE = type(None)
ATOMIC = {"device": int, "cus": int, "cus_seen": int, "values_checked": int, "own_mismatches": int, "shared_mismatches": int, "mismatches": int,
          "bad_cus": int, "bad_cu_keys": int, "first_bad_placement": NONE, "first_bad_class": NONE, "first_bad_op": NONE,
          "first_bad_element": NONE, "first_bad_xor": NONE, "first_bad_delta": NONE, "tickets_out_of_range": int, "f32_add_tbps": float,
          "pk_bf16_add_tbps": float, "u32_add_tbps": float, "rtn_gops": float, "rate_ms": float, "rate_ok": bool, "xcc_waves": int,
          "xcc_us": float, "slowest_xcc": int, "xcc_balance": float, "elapsed_ms": float, "passed": bool}
LISTS = {"own_mismatches": 8, "shared_mismatches": 8, "bad_cu_keys": 0, "rate_ms": 4, "xcc_waves": 8, "xcc_us": 8}
RATES = ("f32_add_tbps", "pk_bf16_add_tbps", "u32_add_tbps", "rtn_gops")
TIMES = RATES + ("rate_ms", "xcc_waves", "xcc_us", "slowest_xcc", "xcc_balance", "elapsed_ms")  # what a clock or the dispatcher decides
CLASSES = ("int32", "int64", "f32", "f64", "pk16", "cas", "ticket", "lds")
RATE_CLASSES = ("f32", "pk_bf16", "u32", "rtn")
CAS_WORD = {"cas": 0, "lds": 8}
TICKET_WORD = {"ticket": 0, "lds": 1}
U32 = np.uint32


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def clean(ops):
    """(result, data) of one clean run: computed once, shared and left unchanged"""
    return ops.atomic_data(seed=SEED, **SMALL)


@pytest.fixture(scope="module")
def referee(ops, clean):
    return ops.atomic_expected(clean[0]["cus"] * SMALL["wgs_per_cu"], ROUNDS, seed=SEED)


def _untimed(r):
    return {k: v for k, v in r.items() if k not in TIMES}


def _mismatches(r):
    return {"own": r["own_mismatches"], "shared": r["shared_mismatches"]}


def _only(placement, cls, n=1):
    return {pl: [n * int(pl == placement and c == cls) for c in CLASSES] for pl in ("own", "shared")}


def _mix32(x):
    x = np.array(x, dtype=U32)
    x ^= x >> U32(16)
    x *= U32(0x7FEB352D)
    x ^= x >> U32(15)
    x *= U32(0x846CA68B)
    x ^= x >> U32(16)
    return x


def _operand(cls, k, wave, rnd, lane):
    """gpu_diag.h, "Atomics": operand word k of (class, wave, round, lane)"""
    return int(_mix32(_mix32(U32(SEED) ^ _mix32(U32(cls << 4 | k))) ^ U32(wave << 12 | rnd << 6 | lane)))


def _row(layout, placement, cls, wave, rnd):
    if placement == "own":
        return 2 * (wave // 4) + (wave + rnd) % 2
    return (wave * ROUNDS + rnd) % int(layout["rows"][1][CLASSES.index(cls)])


def _deterministic(block):
    """every table word whose final value the order of arrival does not decide: all but the cas elements"""
    out = {}
    for pl in ("own", "shared"):
        for cls in CLASSES:
            if cls != "cas":
                out[pl, cls] = block[pl][cls][:8] if cls == "lds" else block[pl][cls]
    return out


def _assert_tables_equal(got, want):
    g, w = _deterministic(got), _deterministic(want)
    for key in g:
        assert np.array_equal(g[key], w[key]), (key, np.argwhere(g[key] != w[key])[:4].tolist())


def _cas_is_sound(block, placement, cls, skip=()):
    """every element has exactly one winner among the lanes whose ballot bit is set, and holds that winner's id"""
    layout = block["layout"]
    elements = block[placement][cls][CAS_WORD[cls]]
    ballots = block["ballots"][2 if cls == "lds" else ("own", "shared").index(placement)]
    pairs = np.arange(int(layout["pairs"]))
    wave, rnd = pairs // ROUNDS, pairs % ROUNDS
    row = 2 * (wave // 4) + (wave + rnd) % 2 if placement == "own" else pairs % elements.shape[0]
    won = (ballots[:, None] >> np.arange(64, dtype=np.uint64)[None, :] & np.uint64(1)).astype(bool)  # [pair, lane]
    count = np.zeros(elements.shape, dtype=np.int64)
    holder = np.zeros(elements.shape, dtype=np.int64)
    lanes = np.broadcast_to(np.arange(64), won.shape)
    rows = np.broadcast_to(row[:, None], won.shape)
    np.add.at(count, (rows[won], lanes[won]), 1)
    np.add.at(holder, (rows[won], lanes[won]), (pairs[:, None] * 64 + lanes)[won])
    bad = np.argwhere((count != 1) | (holder != elements))
    return [tuple(b) for b in bad.tolist() if tuple(b) not in skip]


# ---------------------------------------------------------------------------------------------
# the clean run

def test_clean_run(clean):
    r, d = clean
    print("atomic clean", {k: r[k] for k in ("cus", "cus_seen") + TIMES})
    assert r["own_mismatches"] == [0] * 8 and r["shared_mismatches"] == [0] * 8 and r["mismatches"] == 0
    assert r["bad_cus"] == 0 and r["bad_cu_keys"] == [] and r["tickets_out_of_range"] == 0
    assert r["rate_ok"] is True and r["passed"] is True and 0 < r["cus_seen"] <= r["cus"]
    assert all(math.isfinite(r[k]) and r[k] > 0 for k in RATES) and all(math.isfinite(ms) and ms > 0 for ms in r["rate_ms"])
    assert sum(r["xcc_waves"]) == 4 * 4 * ((2 * r["cus"] + 7) // 8 * 8) and 0 < r["xcc_balance"] <= 1 and 0 <= r["slowest_xcc"] < 8
    assert r["elapsed_ms"] >= sum(r["rate_ms"])
    assert ((0 <= d["cu_keys"]) & (d["cu_keys"] < 2048)).all() and len(set(d["cu_keys"].tolist())) == r["cus_seen"]
    assert ((0 <= d["rate_cu_keys"]) & (d["rate_cu_keys"] < 2048)).all()


def test_result_shape(clean):
    r = clean[0]
    assert list(r) == list(ATOMIC)
    wrong = {k: type(r[k]).__name__ for k in ATOMIC if k not in LISTS and type(r[k]) is not ATOMIC[k]}
    assert not wrong, wrong
    for k, n in LISTS.items():
        assert type(r[k]) is list and len(r[k]) == n and all(type(v) is ATOMIC[k] for v in r[k]), k


def test_the_tables_equal_the_referee_word_for_word(clean, referee):
    d = clean[1]
    assert d["words"].size == referee["words"].size - 32 + 4 * d["rate_cu_keys"].shape[1]  # the referee's rate grid is 8
    _assert_tables_equal(d, referee)
    for placement, cls in (("own", "cas"), ("shared", "cas"), ("own", "lds")):
        assert _cas_is_sound(d, placement, cls) == [], (placement, cls)
    assert np.array_equal(d["own"]["ticket"][0], np.full(d["own"]["ticket"][0].shape, 2 * ROUNDS))


def test_every_ticket_was_drawn_once(clean, referee):
    r, d = clean
    assert r["tickets_out_of_range"] == 0
    for which in ("own", "shared", "lds"):
        got, want = np.sort(d["order"][which], axis=2), np.sort(referee["order"][which], axis=2)
        assert np.array_equal(got, want), (which, np.argwhere(got != want)[:4].tolist())
        assert (want[:, :, -1] > 0).all()  # every element has pullers


def test_one_more_iteration_visits_one_more_row(ops, clean):
    r = ops.atomic(seed=SEED, **dict(SMALL, rate_iters=16))
    assert r["rate_ok"] is True and r["passed"] is True and r["mismatches"] == 0
    assert _untimed(r) == _untimed(clean[0])


def test_planted_and_delayed_variants_without_plants_are_the_same_run(ops, clean):
    for r in (ops.atomic_planted([], [], seed=SEED, **SMALL), ops.atomic_delayed([], seed=SEED, **SMALL)):
        assert list(r) == list(ATOMIC)
        assert _untimed(r) == _untimed(clean[0])


# ---------------------------------------------------------------------------------------------
# lost and doubled updates

ADDS = [(pl, cls, k) for pl in ("own", "shared") for cls, k in (("int32", 0), ("int32", 5), ("int64", 0), ("f32", 0), ("f64", 0), ("pk16", 0), ("pk16", 1))]
ADDS += [("own", "lds", 0), ("own", "lds", 6), ("own", "lds", 7)]
XORS = {("int32", 5), ("lds", 6)}  # a doubled xor cancels itself: only the lost one can show
ADD_CASES = [(pl, cls, k, times) for pl, cls, k in ADDS for times in (0, 2) if not (times == 2 and (cls, k) in XORS)]


def _value(cls, k, word):
    """a table word as the number it holds (pk16: the pair of its halves)"""
    if cls == "f32" or (cls == "lds" and k == 7):
        return int(np.array(word, dtype=U32).view(np.float32))
    if cls == "f64":
        return int(np.array(word, dtype=np.uint64).view(np.float64))
    if cls == "pk16":
        halves = np.array([int(word) & 0xFFFF, int(word) >> 16], dtype=np.uint16)
        return tuple(int(v) for v in ((halves.astype(U32) << U32(16)).view(np.float32) if k == 0 else halves.view(np.float16)))
    return int(word)


def _signed(x, bits):
    x %= 1 << bits
    return x - (1 << bits) if x >> (bits - 1) else x


@pytest.mark.parametrize("placement,cls,k,times", ADD_CASES, ids=[f"{pl}-{cls}-{k}-{('lost', 0, 'doubled')[t]}" for pl, cls, k, t in ADD_CASES])
def test_a_lost_and_a_doubled_update_give_one_wrong_word_off_by_the_operand(ops, clean, referee, placement, cls, k, times):
    cus = clean[0]["cus"]
    wave, rnd = (4 * cus - 1, 1) if times == 0 else (5, 0)
    # a lane whose operand is not 0 (a trit, or a float of the f32 classes, may be): the referee must show the plant
    for lane in (37, 38, 39, 40, 41, 42):
        plant = (placement, cls, k, wave, rnd, lane, times, 0)
        want = ops.atomic_expected(cus, ROUNDS, plants=[plant], seed=SEED)
        if np.count_nonzero(want["words"] != referee["words"]):
            break
    row = _row(want["layout"], placement, cls, wave, rnd)
    at = (row, lane) if cls in ("int64", "f64") else (k, row, lane)
    before, after = referee[placement][cls][at], want[placement][cls][at]
    assert before != after and np.count_nonzero(want[placement][cls] != referee[placement][cls]) == 1
    r, d = ops.atomic_data(plants=[plant], seed=SEED, **SMALL)
    _assert_tables_equal(d, want)  # the device did what the referee did with the same plant: one word moved, by the operand
    assert _mismatches(r) == _only(placement, cls) and r["mismatches"] == 1 and r["passed"] is False
    assert (r["first_bad_placement"], r["first_bad_class"], r["first_bad_op"], r["first_bad_element"]) == (placement, cls, k, row * 64 + lane)
    assert int(r["first_bad_xor"], 16) == int(before) ^ int(after)
    if (cls, k) in XORS:
        assert r["first_bad_delta"] == 0 and int(before) ^ int(after) == _operand(CLASSES.index(cls), k, wave, rnd, lane)
    elif cls == "pk16":
        (lo0, hi0), (lo1, hi1) = _value(cls, k, before), _value(cls, k, after)
        assert r["first_bad_delta"] == (lo1 - lo0 if lo1 != lo0 else hi1 - hi0) and abs(r["first_bad_delta"]) == 1
    else:
        delta = _value(cls, k, after) - _value(cls, k, before)
        assert r["first_bad_delta"] == (_signed(delta, 32) if cls in ("int32", "lds") and k == 0 else _signed(delta, 64) if cls == "int64" else delta)
    if placement == "own":  # the CU that the planted workgroup itself recorded in this run
        assert r["bad_cus"] == 1 and r["bad_cu_keys"] == [int(d["cu_keys"][wave // 4])]
    else:
        assert r["bad_cus"] == 0 and r["bad_cu_keys"] == []
    assert r["rate_ok"] is True and r["tickets_out_of_range"] == 0
    assert r["values_checked"] == clean[0]["values_checked"] and r["cus_seen"] == clean[0]["cus_seen"]


# ---------------------------------------------------------------------------------------------
# operations that a repeat does not change: a wrong operand that dominates

DOMINANT = {"smin": 0x80000000, "umax": 0xFFFFFFFF, "and": 0x00000000, "or": 0xFFFFFFFF}
IDEMPOTENT = [(pl, "int32", k, name) for pl in ("own", "shared") for k, name in ((1, "smin"), (2, "umax"), (3, "and"), (4, "or"))]
IDEMPOTENT += [("own", "lds", k, name) for k, name in ((3, "smin"), (2, "umax"), (4, "and"), (5, "or"))]


@pytest.mark.parametrize("placement,cls,k,name", IDEMPOTENT, ids=[f"{pl}-{cls}-{name}" for pl, cls, k, name in IDEMPOTENT])
def test_a_dominating_operand_shows_where_the_referee_says_it_must(ops, clean, referee, placement, cls, k, name):
    cus = clean[0]["cus"]
    wave, rnd = 4 * cus - 2, 1
    row = _row(referee["layout"], placement, cls, wave, rnd)
    # a lane on which the referee shows the plant: an `and` of the 4 operands of an OWN element may be 0 already
    for lane in (63, 62, 61, 60, 59, 58):
        mask = _operand(CLASSES.index(cls), k, wave, rnd, lane) ^ DOMINANT[name]
        assert mask != 0
        plant = (placement, cls, k, wave, rnd, lane, 1, mask)
        want = ops.atomic_expected(cus, ROUNDS, plants=[plant], seed=SEED)
        shows = int(want[placement][cls][k, row, lane]) != int(referee[placement][cls][k, row, lane])
        if shows:
            break
    saturated = placement == "shared" and name in ("and", "or")  # 2048 hashed operands: the word is 0 or all ones already
    assert shows is not saturated
    if shows:
        assert int(want[placement][cls][k, row, lane]) == DOMINANT[name]
    r, d = ops.atomic_data(plants=[plant], seed=SEED, **SMALL)
    _assert_tables_equal(d, want)
    if not shows:
        assert _untimed(r) == _untimed(clean[0])
        return
    assert _mismatches(r) == _only(placement, cls) and r["passed"] is False
    assert (r["first_bad_placement"], r["first_bad_class"], r["first_bad_op"], r["first_bad_element"]) == (placement, cls, k, row * 64 + lane)
    assert int(r["first_bad_xor"], 16) == int(referee[placement][cls][k, row, lane]) ^ DOMINANT[name] and r["first_bad_delta"] == 0
    assert r["bad_cu_keys"] == ([int(d["cu_keys"][wave // 4])] if placement == "own" else [])


@pytest.mark.parametrize("placement,cls", [("own", "cas"), ("shared", "cas"), ("own", "lds")])
def test_a_wrong_id_on_every_contender_of_one_cas_element(ops, clean, placement, cls):
    """whoever wins the element then holds a wrong id: one wrong element, the others sound"""
    r0, d0 = clean
    layout, lane, mask = d0["layout"], 11, 0x40000000
    wave0 = 4 * r0["cus"] - 4  # the last workgroup's first wave, round 0
    row = _row(layout, placement, cls, wave0, 0)
    contenders = [(w, rnd) for w in range(int(layout["waves"])) for rnd in range(ROUNDS) if _row(layout, placement, cls, w, rnd) == row]
    assert len(contenders) == (2 * ROUNDS if placement == "own" else int(layout["order_cap"][1]))
    r, d = ops.atomic_data(plants=[(placement, cls, CAS_WORD[cls], w, rnd, lane, 1, mask) for w, rnd in contenders], seed=SEED, **SMALL)
    assert _mismatches(r) == _only(placement, cls) and r["passed"] is False
    assert (r["first_bad_placement"], r["first_bad_class"], r["first_bad_op"], r["first_bad_element"]) == (placement, cls, CAS_WORD[cls], row * 64 + lane)
    assert _cas_is_sound(d, placement, cls, skip=[(row, lane)]) == []
    held = int(d[placement][cls][CAS_WORD[cls]][row, lane])
    assert held & mask and ((held ^ mask) // 64 // ROUNDS, (held ^ mask) // 64 % ROUNDS) in contenders and (held ^ mask) % 64 == lane
    assert r["bad_cu_keys"] == ([int(d["cu_keys"][wave0 // 4])] if placement == "own" else [])


@pytest.mark.parametrize("times", [0, 2], ids=["lost", "doubled"])
@pytest.mark.parametrize("placement,cls", [("own", "ticket"), ("shared", "ticket"), ("own", "lds")])
def test_a_lost_and_a_doubled_pull_of_a_ticket(ops, clean, referee, placement, cls, times):
    cus = clean[0]["cus"]
    wave, rnd, lane, k = 4 * cus - 3, 1, 20, TICKET_WORD[cls]
    r, d = ops.atomic_data(plants=[(placement, cls, k, wave, rnd, lane, times, 0)], seed=SEED, **SMALL)
    row = _row(d["layout"], placement, cls, wave, rnd)
    pullers = int(referee[placement][cls][k, row, lane])
    which = "lds" if cls == "lds" else placement
    drawn, ids = d["order"][which][row, lane], referee["order"][which][row, lane]
    mine = (wave * ROUNDS + rnd) * 64 + lane + 1
    assert mine in ids.tolist()
    assert int(d[placement][cls][k, row, lane]) == pullers + times - 1  # the counter is one short, or one over
    if times == 0:  # one id is missing and every other one is there once
        assert r["tickets_out_of_range"] == 0
        assert sorted(drawn.tolist()) == sorted([0] + [i for i in ids.tolist() if i != mine])
    else:  # the array is full, so one pull drew a ticket at its capacity: counted, and nothing stored
        assert r["tickets_out_of_range"] == 1
        twice = drawn.tolist().count(mine) - 1  # 0 if the dropped pull was one of the lane's own two, 1 if it was another lane's
        assert twice in (0, 1) and set(drawn.tolist()) <= set(ids.tolist()) and len(set(drawn.tolist())) == len(ids) - twice
    assert _mismatches(r) == _only(placement, cls) and r["passed"] is False
    assert (r["first_bad_placement"], r["first_bad_class"], r["first_bad_op"], r["first_bad_element"]) == (placement, cls, k, row * 64 + lane)
    assert r["bad_cu_keys"] == ([int(d["cu_keys"][wave // 4])] if placement == "own" else [])


def test_a_plant_beyond_the_launch_is_refused(ops, clean):
    waves, rate_waves = 4 * clean[0]["cus"], 4 * ((2 * clean[0]["cus"] + 7) // 8 * 8)
    beyond = "atomic diag: invalid arguments: plant in a wave beyond the launch"
    with pytest.raises(RuntimeError, match=beyond):
        ops.atomic_planted([("own", "int32", 0, waves, 0, 0, 0, 0)], [], seed=SEED, **SMALL)
    with pytest.raises(RuntimeError, match=beyond):
        ops.atomic_planted([], [("f32", 0, 0, 0), ("u32", rate_waves, 0, 2)], seed=SEED, **SMALL)
    with pytest.raises(RuntimeError, match=beyond):
        ops.atomic_delayed([("rtn", rate_waves, 1)], seed=SEED, **SMALL)
    with pytest.raises(RuntimeError, match=beyond):
        ops.atomic_data(plants=[("shared", "f64", 0, waves + 7, 1, 63, 2, 0)], seed=SEED, **SMALL)


# ---------------------------------------------------------------------------------------------
# the rate phase

@pytest.mark.parametrize("iters", [15, 16])
@pytest.mark.parametrize("cls", RATE_CLASSES)
def test_a_rate_plant_clears_rate_ok_and_nothing_else(ops, clean, cls, iters):
    rate_waves = 4 * ((2 * clean[0]["cus"] + 7) // 8 * 8)
    if cls in ("f32", "pk_bf16"):  # a lane's trit may be 0: every lane of the wave loses its last add (all 64 are 0 once in 3^64)
        plants = [(cls, rate_waves - 1, lane, 0) for lane in range(64)]
    elif cls == "u32":
        plants = [(cls, 0, 63, 2)]
    else:
        plants = [(cls, rate_waves - 1, 0, 0)]
    r = ops.atomic_planted([], plants, seed=SEED, **dict(SMALL, rate_iters=iters))
    assert r["rate_ok"] is False and r["passed"] is False
    assert _untimed(dict(r, rate_ok=True, passed=True)) == _untimed(clean[0])


T = 2_000_000  # ticks of the constant clock
CLOCK_KHZ = 100_000  # CDNA's constant clock: 100 MHz


def test_a_delayed_wave_shows_in_its_class_and_names_its_xcc(ops, clean):
    c = clean[0]
    wave = 4 * ((2 * c["cus"] + 7) // 8 * 8) - 1
    r, d = ops.atomic_data(delays=[("f32", wave, T)], seed=SEED, **SMALL)
    print("atomic delayed", {k: r[k] for k in TIMES}, "ran on", d["rate_cu_keys"][:, wave // 4], "clean", {k: c[k] for k in TIMES})
    assert r["rate_ms"][0] >= T / CLOCK_KHZ  # the launch cannot end before its wave's 20 ms: derived, not measured
    assert r["f32_add_tbps"] <= (wave + 1) * 64 * 4 * SMALL["rate_iters"] / (T / CLOCK_KHZ * 1e-3) / 1e12
    # the XCC that the wave recorded in that class's timed launch of this run has waited 20 ms more than any other
    key = int(d["rate_cu_keys"][0, wave // 4])
    assert 0 <= key < 2048 and r["slowest_xcc"] == key >> 8
    assert r["xcc_us"][key >> 8] >= T / (CLOCK_KHZ / 1e3) / r["xcc_waves"][key >> 8]  # its share of the mean over that XCC's waves
    assert r["xcc_balance"] < c["xcc_balance"]
    assert _untimed(r) == _untimed(c)  # nothing else moves: no value is touched
    _assert_tables_equal(d, clean[1])


def test_the_delayed_entry_shows_the_delay_alike(ops, clean):
    r = ops.atomic_delayed([("f32", 3, T)], seed=SEED, **SMALL)
    assert r["rate_ms"][0] >= T / CLOCK_KHZ and 0 <= r["slowest_xcc"] < 8
    assert _untimed(r) == _untimed(clean[0])
