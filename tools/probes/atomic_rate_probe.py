"""Atomic rates and the cost of the atomic check of the diagnostics on the MI355X.  Writes the runs as JSON.

    python3 tools/probes/atomic_rate_probe.py rates out.json     # 12 runs back to back per point
    python3 tools/probes/atomic_rate_probe.py pass out.json      # one whole pass; run it in a fresh process
    python3 tools/probes/atomic_rate_probe.py summary rates.json pass1.json ... out.json   # needs no GPU

* rates: ops.atomic() at 1, 2, 4 and 8 workgroups per CU of the check and 1023, 4095 and 16383 rate iterations, each
  run right after ops.mfma(), so the clocks are as in a pass; then 12 runs at ops.atomic()'s defaults and one at the
  largest arguments (8 workgroups per CU, 64 rounds, 65536 iterations).  Every run records the four rates, the time of
  each timed launch, of the check launch and of all kernels together, the wall time of the call, which includes
  the copies and the host referee, the XCCs' mean loop times and the verdict (RUN_KEYS).
* pass: hbm, mfma, mfma_lowp, mfma_classic, lds, cache, valu and atomic at their defaults, once, as a node agent's
  pass would order them: the rates that a floor has to hold against.
* summary: the `rates` file and the `pass` files as one record: the range of every rate, time and balance per point,
  the lowest run of each rate at the defaults and the floor 25 % under it.
  profiles/atomic_diag/rates.json is this, made from the files in profiles/atomic_diag/raw/.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from bacchus_gpu_controller_amd import ops  # noqa: E402

RUNS = 12
RATES = ("f32_add_tbps", "pk_bf16_add_tbps", "u32_add_tbps", "rtn_gops")
LARGEST = dict(wgs_per_cu=8, rounds=64, rate_iters=65536)


def write(path, record):
    """JSON with one line per top-level entry, and one per element of a top-level list: a run, a point or a section is a line"""
    def value(v):
        if isinstance(v, list) and v and isinstance(v[0], dict):
            return "[\n  " + ",\n  ".join(json.dumps(x) for x in v) + "\n ]"
        return json.dumps(v)

    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {value(v)}" for k, v in record.items()) + "\n}\n")


RUN_KEYS = ("label", "wgs_per_cu", "rounds", "rate_iters") + RATES + (
    "rate_ms", "check_ms", "elapsed_ms", "wall_ms", "cus_seen", "xcc_us", "xcc_balance", "slowest_xcc", "values_checked", "mismatches",
    "tickets_out_of_range", "rate_ok", "passed", "mfma_tflops")


def trimmed(r):
    """what a run records: the keys above, times and rates to 5 decimals"""
    def short(v):
        return round(v, 5) if isinstance(v, float) else [short(x) for x in v] if isinstance(v, list) else v

    return {k: short(r[k]) for k in RUN_KEYS if k in r}


def one(label, **args):
    m = ops.mfma(0, 16, 2048)
    t0 = time.time()
    r = ops.atomic(0, **args)
    r.update(label=label, wall_ms=round((time.time() - t0) * 1e3, 2), check_ms=round(r["elapsed_ms"] - sum(r["rate_ms"]), 4),
             mfma_tflops=m["tflops"], **args)
    return trimmed(r)


def show(r):
    print(r["label"], r["wgs_per_cu"], r["rounds"], r["rate_iters"], [round(r[k], 3) for k in RATES], [round(ms, 3) for ms in r["rate_ms"]],
          r["check_ms"], round(r["elapsed_ms"], 3), r["wall_ms"], r["cus_seen"], round(r["xcc_balance"], 3), r["passed"], flush=True)


def rates(path):
    runs = []
    points = [(wgs, iters) for wgs in (1, 2, 4, 8) for iters in (1023, 4095, 16383)]
    points.append((ops.ATOMIC_WGS_PER_CU, ops.ATOMIC_RATE_ITERS))
    for i, (wgs, iters) in enumerate(points):
        label = "defaults" if i == len(points) - 1 else "sweep"
        for _ in range(RUNS):
            runs.append(one(label, wgs_per_cu=wgs, rounds=ops.ATOMIC_ROUNDS, rate_iters=iters))
            show(runs[-1])
    runs.append(one("largest", **LARGEST))
    show(runs[-1])
    write(path, {"runs": runs})
    return 0 if all(r["passed"] for r in runs) else 1


def whole_pass(path):
    out = {}
    for name, fn in (("hbm", lambda: ops.hbm(0, nbytes=1 << 30)), ("mfma", lambda: ops.mfma(0)), ("mfma_lowp", lambda: ops.mfma_lowp(0)),
                     ("mfma_classic", lambda: ops.mfma_classic(0)), ("lds", lambda: ops.lds(0)), ("cache", lambda: ops.cache(0)),
                     ("valu", lambda: ops.valu(0)), ("atomic", lambda: ops.atomic(0))):
        t0 = time.time()
        out[name] = fn()
        out[name]["wall_ms"] = round((time.time() - t0) * 1e3, 2)
    a = out["atomic"]
    a.update(label="pass", check_ms=round(a["elapsed_ms"] - sum(a["rate_ms"]), 4), wgs_per_cu=ops.ATOMIC_WGS_PER_CU, rounds=ops.ATOMIC_ROUNDS,
             rate_iters=ops.ATOMIC_RATE_ITERS)
    show(a)
    write(path, out)
    return 0 if all(r["passed"] for r in out.values()) else 1


WHAT = ("tools/probes/atomic_rate_probe.py on one MI355X (gfx950, 256 CUs): `rates` (12 runs back to back per point, each right after ops.mfma, "
        "and one run at the largest arguments) and `pass` (hbm, mfma, mfma_lowp, mfma_classic, lds, cache, valu, atomic at their defaults in a "
        "fresh process), joined by `summary`")


def summary(rates_path, *rest):
    *pass_paths, out_path = rest
    with open(rates_path) as f:
        runs = json.load(f)["runs"]
    groups = {}
    for r in runs:
        groups.setdefault((r["label"], r["wgs_per_cu"], r["rounds"], r["rate_iters"]), []).append(r)

    def span(v, key, digits):
        return [round(min(r[key] for r in v), digits), round(max(r[key] for r in v), digits)]

    points = []
    for (label, wgs, rounds, iters), v in groups.items():
        p = {"label": label, "wgs_per_cu": wgs, "rounds": rounds, "rate_iters": iters, "runs": len(v)}
        p.update({k: span(v, k, 3) for k in RATES})
        p.update(check_ms=span(v, "check_ms", 3), elapsed_ms=span(v, "elapsed_ms", 3), wall_ms=span(v, "wall_ms", 2),
                 xcc_balance=span(v, "xcc_balance", 3), cus_seen=sorted({r["cus_seen"] for r in v}), all_passed=all(r["passed"] for r in v))
        points.append(p)
    passes = []
    for path in pass_paths:
        with open(path) as f:
            v = json.load(f)
        passes.append({"atomic": trimmed(v["atomic"]),
                       "before_it": {"l2_read_tbps": v["cache"]["l2_read_tbps"], "valu_fp32_tflops": v["valu"]["fp32_tflops"]}})
    defaults = {"wgs_per_cu": ops.ATOMIC_WGS_PER_CU, "rounds": ops.ATOMIC_ROUNDS, "rate_iters": ops.ATOMIC_RATE_ITERS}
    at_defaults = [r for r in runs if all(r[k] == v for k, v in defaults.items())]
    lowest = {k: min([r[k] for r in at_defaults] + [p["atomic"][k] for p in passes]) for k in RATES}
    out = {"what": WHAT,
           "units": {"f32_add_tbps": "TB/s of added bytes, global_atomic_add_f32 without return", "pk_bf16_add_tbps": "TB/s, global_atomic_pk_add_bf16",
                     "u32_add_tbps": "TB/s, global_atomic_add", "rtn_gops": "10^9 returning global_atomic_add per second, one lane per wave"},
           "defaults": defaults, "lowest_run_at_defaults": {k: round(v, 3) for k, v in lowest.items()},
           "proposed_floors_25_percent_under_lowest": {k: round(0.75 * v, 2) for k, v in lowest.items()},
           "points": points, "fresh_process_passes": passes}
    write(out_path, out)
    print(out["lowest_run_at_defaults"], out["proposed_floors_25_percent_under_lowest"])
    return 0


if __name__ == "__main__":
    sys.exit({"rates": rates, "pass": whole_pass, "summary": summary}[sys.argv[1]](*sys.argv[2:]))
