"""Move rate and cost of the register-file check of the diagnostics on the MI355X.  Writes the runs as JSON.

    python3 tools/probes/regfile_rate_probe.py rates out.json     # 12 runs back to back per point
    python3 tools/probes/regfile_rate_probe.py pass out.json      # one whole pass; run it in a fresh process
    python3 tools/probes/regfile_rate_probe.py summary rates.json pass1.json ... out.json   # needs no GPU

* rates: ops.regfile() at 1 and 2 workgroups per CU and 256, 1024, 4096 and 16384 sweeps, each run right after
  ops.mfma(), so the clocks are as in a pass; then 12 runs at ops.regfile()'s defaults.  Every run records the move
  rate, the SIMD balance, the time of the march launch and of the timed rotate launch, the wall time of the call,
  which includes the copies and the host's fold, and the verdict (RUN_KEYS).
* pass: hbm, mfma, mfma_lowp, mfma_classic, lds, cache, valu, atomic and regfile at their defaults, once, as a node
  agent's pass would order them: the rate that a floor has to hold against.
* summary: the `rates` file and the `pass` files as one record: the range of the rate, the times and the balance per
  point, the lowest run at the defaults, the floor 25 % under it and the rate's share of the issue ceiling of one wave
  per SIMD (CUs * 4 SIMDs * 16 lanes per clock at 2.4 GHz).
  profiles/regfile_diag/rates.json is this, made from the files in profiles/regfile_diag/raw/.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from bacchus_gpu_controller_amd import ops  # noqa: E402

RUNS = 12
CLOCK_GHZ = 2.4
RUN_KEYS = ("label", "wgs_per_cu", "sweeps", "mov_tops", "simd_balance", "march_ms", "rotate_ms", "elapsed_ms", "wall_ms", "cus", "cus_seen",
            "simds_seen", "slowest_cu_key", "slowest_simd", "words_checked", "mismatches", "rate_ok", "passed", "mfma_tflops")


def write(path, record):
    """JSON with one line per top-level entry, and one per element of a top-level list: a run, a point or a section is a line"""
    def value(v):
        if isinstance(v, list) and v and isinstance(v[0], dict):
            return "[\n  " + ",\n  ".join(json.dumps(x) for x in v) + "\n ]"
        return json.dumps(v)

    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {value(v)}" for k, v in record.items()) + "\n}\n")


def trimmed(r):
    """what a run records: the keys above, times and rates to 5 decimals"""
    return {k: round(r[k], 5) if isinstance(r[k], float) else r[k] for k in RUN_KEYS if k in r}


def one(label, **args):
    m = ops.mfma(0, 16, 2048)
    t0 = time.time()
    r = ops.regfile(0, **args)
    r.update(label=label, wall_ms=round((time.time() - t0) * 1e3, 2), mfma_tflops=m["tflops"], **args)
    return trimmed(r)


def show(r):
    print(r["label"], r["wgs_per_cu"], r["sweeps"], round(r["mov_tops"], 3), round(r["simd_balance"], 3), round(r["march_ms"], 3),
          round(r["rotate_ms"], 3), r["wall_ms"], r["simds_seen"], r["passed"], flush=True)


def rates(path):
    runs = []
    points = [(wgs, sweeps) for wgs in (1, 2) for sweeps in (256, 1024, 4096, 16384)]
    points.append((ops.REGFILE_WGS_PER_CU, ops.REGFILE_SWEEPS))
    for i, (wgs, sweeps) in enumerate(points):
        label = "defaults" if i == len(points) - 1 else "sweep"
        for _ in range(RUNS):
            runs.append(one(label, wgs_per_cu=wgs, sweeps=sweeps))
            show(runs[-1])
    write(path, {"runs": runs})
    return 0 if all(r["passed"] for r in runs) else 1


def whole_pass(path):
    out = {}
    for name, fn in (("hbm", lambda: ops.hbm(0, nbytes=1 << 30)), ("mfma", lambda: ops.mfma(0)), ("mfma_lowp", lambda: ops.mfma_lowp(0)),
                     ("mfma_classic", lambda: ops.mfma_classic(0)), ("lds", lambda: ops.lds(0)), ("cache", lambda: ops.cache(0)),
                     ("valu", lambda: ops.valu(0)), ("atomic", lambda: ops.atomic(0)), ("regfile", lambda: ops.regfile(0))):
        t0 = time.time()
        out[name] = fn()
        out[name]["wall_ms"] = round((time.time() - t0) * 1e3, 2)
    out["regfile"].update(label="pass", wgs_per_cu=ops.REGFILE_WGS_PER_CU, sweeps=ops.REGFILE_SWEEPS)
    show(out["regfile"])
    write(path, out)
    return 0 if all(r["passed"] for r in out.values()) else 1


WHAT = ("tools/probes/regfile_rate_probe.py on one MI355X (gfx950, 256 CUs): `rates` (12 runs back to back per point, each right after ops.mfma) "
        "and `pass` (hbm, mfma, mfma_lowp, mfma_classic, lds, cache, valu, atomic, regfile at their defaults in a fresh process), joined by `summary`")


def summary(rates_path, *rest):
    *pass_paths, out_path = rest
    with open(rates_path) as f:
        runs = json.load(f)["runs"]
    groups = {}
    for r in runs:
        groups.setdefault((r["label"], r["wgs_per_cu"], r["sweeps"]), []).append(r)

    def span(v, key, digits):
        return [round(min(r[key] for r in v), digits), round(max(r[key] for r in v), digits)]

    points = []
    for (label, wgs, sweeps), v in groups.items():
        p = {"label": label, "wgs_per_cu": wgs, "sweeps": sweeps, "runs": len(v)}
        p.update(mov_tops=span(v, "mov_tops", 3), simd_balance=span(v, "simd_balance", 3), march_ms=span(v, "march_ms", 3),
                 rotate_ms=span(v, "rotate_ms", 3), wall_ms=span(v, "wall_ms", 2), simds_seen=sorted({r["simds_seen"] for r in v}),
                 all_passed=all(r["passed"] for r in v))
        points.append(p)
    passes = []
    for path in pass_paths:
        with open(path) as f:
            v = json.load(f)
        passes.append({"regfile": trimmed(v["regfile"]),
                       "before_it": {"valu_fp32_tflops": v["valu"]["fp32_tflops"], "atomic_u32_add_tbps": v["atomic"]["u32_add_tbps"]}})
    defaults = {"wgs_per_cu": ops.REGFILE_WGS_PER_CU, "sweeps": ops.REGFILE_SWEEPS}
    at_defaults = [r for r in runs if all(r[k] == v for k, v in defaults.items())] + [p["regfile"] for p in passes]
    lowest = min(r["mov_tops"] for r in at_defaults)
    ceiling = at_defaults[0]["cus"] * 4 * 16 * CLOCK_GHZ * 1e9 / 1e12
    out = {"what": WHAT,
           "units": {"mov_tops": "10^12 lane-moves per second of the timed rotate: waves * 64 lanes * 504 ring registers * sweeps / rotate_ms",
                     "simd_balance": "fastest / slowest (CU, SIMD) mean loop time", "march_ms": "device time of the march launch",
                     "rotate_ms": "device time of the timed rotate launch"},
           "defaults": defaults, "issue_ceiling_tops_at_2.4_ghz": round(ceiling, 2),
           "lowest_run_at_defaults": {"mov_tops": round(lowest, 3), "share_of_ceiling": round(lowest / ceiling, 3)},
           "proposed_floors_25_percent_under_lowest": {"mov_tops": round(0.75 * lowest, 1)},
           "at_defaults": {k: span(at_defaults, k, 3) for k in ("mov_tops", "simd_balance", "march_ms", "rotate_ms")},
           "points": points, "fresh_process_passes": passes}
    write(out_path, out)
    print(out["lowest_run_at_defaults"], out["proposed_floors_25_percent_under_lowest"])
    return 0


if __name__ == "__main__":
    sys.exit({"rates": rates, "pass": whole_pass, "summary": summary}[sys.argv[1]](*sys.argv[2:]))
