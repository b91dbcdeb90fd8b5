"""Cross-lane rates of the diagnostics on the MI355X.  Writes the runs as JSON.

    python3 tools/probes/xlane_rate_probe.py rates out.json     # 12 runs back to back per point
    python3 tools/probes/xlane_rate_probe.py pass out.json      # one whole pass; run it in a fresh process
    python3 tools/probes/xlane_rate_probe.py summary rates.json pass1.json ... out.json   # needs no GPU

* rates: ops.xlane() at 1, 2, 4 and 8 waves per SIMD and 1024, 4096 and 16384 rate iterations, each run
  right after ops.mfma(), so the clocks are as in a pass; then 12 runs at ops.xlane()'s defaults.  Every
  run records the four rates, the time of each timed launch and of all kernels together, and the wall
  time of the call.
* pass: hbm, mfma, mfma_lowp, mfma_classic, lds, cache, valu and xlane at their defaults, once, as a node
  agent's pass would order them: the rates that a floor has to hold against.
* summary: the `rates` file and the `pass` files as one record: the range of every rate, time and balance per
  point, the runs at the defaults, the lowest run of each rate there and the floor 25 % under it.
  profiles/xlane_diag/rates.json is this, made from the files in profiles/xlane_diag/raw/.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from bacchus_gpu_controller_amd import ops  # noqa: E402

RUNS = 12
RATES = ("dpp_tops", "swap_tops", "bpermute_tops", "swizzle_tops")


def one(label, **args):
    m = ops.mfma(0, 16, 2048)
    t0 = time.time()
    r = ops.xlane(0, **args)
    r.update(label=label, wall_ms=round((time.time() - t0) * 1e3, 2), mfma_tflops=m["tflops"], **args)
    return r


def rates(path):
    runs = []
    points = [(wps, iters) for wps in (1, 2, 4, 8) for iters in (1024, 4096, 16384)]
    points.append((ops.XLANE_WAVES_PER_SIMD, ops.XLANE_RATE_ITERS))
    for i, (wps, iters) in enumerate(points):
        label = "defaults" if i == len(points) - 1 else "sweep"
        for _ in range(RUNS):
            r = one(label, waves_per_simd=wps, rounds=ops.XLANE_ROUNDS, rate_iters=iters)
            runs.append(r)
            print(label, wps, iters, [round(r[k], 2) for k in RATES], [round(ms, 3) for ms in r["rate_ms"]], round(r["elapsed_ms"], 3),
                  r["wall_ms"], r["cus_seen"], r["simds_seen"], r["cu_balance"], r["passed"], flush=True)
    with open(path, "w") as f:
        json.dump({"runs": runs}, f, indent=1)
    return 0 if all(r["passed"] for r in runs) else 1


def whole_pass(path):
    out = {}
    for name, fn in (("hbm", lambda: ops.hbm(0, nbytes=1 << 30)), ("mfma", lambda: ops.mfma(0)), ("mfma_lowp", lambda: ops.mfma_lowp(0)),
                     ("mfma_classic", lambda: ops.mfma_classic(0)), ("lds", lambda: ops.lds(0)), ("cache", lambda: ops.cache(0)),
                     ("valu", lambda: ops.valu(0)), ("xlane", lambda: ops.xlane(0))):
        t0 = time.time()
        out[name] = fn()
        out[name]["wall_ms"] = round((time.time() - t0) * 1e3, 2)
    v = out["xlane"]
    print("pass", [round(v[k], 2) for k in RATES], [round(ms, 3) for ms in v["rate_ms"]], round(v["elapsed_ms"], 3), v["wall_ms"], v["passed"],
          flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    return 0 if all(r["passed"] for r in out.values()) else 1


SUMMARY_KEYS = ("label", "waves_per_simd", "rounds", "rate_iters") + RATES + (
    "rate_ms", "elapsed_ms", "wall_ms", "cus_seen", "simds_seen", "cu_balance", "slowest_cu_key", "values_checked", "mismatches", "rate_ok",
    "passed", "mfma_tflops")
WHAT = ("tools/probes/xlane_rate_probe.py on one MI355X (gfx950, 256 CUs): `rates` (12 runs back to back per point, each right after "
        "ops.mfma) and `pass` (hbm, mfma, mfma_lowp, mfma_classic, lds, cache, valu, xlane at their defaults in a fresh process), joined by "
        "`summary`")


def summary(rates_path, *rest):
    *pass_paths, out_path = rest
    with open(rates_path) as f:
        runs = json.load(f)["runs"]
    groups = {}
    for r in runs:
        groups.setdefault((r["label"], r["waves_per_simd"], r["rate_iters"]), []).append(r)

    def span(v, key, digits):
        return [round(min(r[key] for r in v), digits), round(max(r[key] for r in v), digits)]

    points = []
    for (label, wps, iters), v in groups.items():
        p = {"label": label, "waves_per_simd": wps, "rounds": v[0]["rounds"], "rate_iters": iters, "runs": len(v)}
        p.update({k: span(v, k, 2) for k in RATES})
        p.update(elapsed_ms=span(v, "elapsed_ms", 3), wall_ms=span(v, "wall_ms", 2), cu_balance=span(v, "cu_balance", 3),
                 cus_seen=sorted({r["cus_seen"] for r in v}), simds_seen=sorted({r["simds_seen"] for r in v}),
                 all_passed=all(r["passed"] for r in v))
        points.append(p)
    passes = []
    for path in pass_paths:
        with open(path) as f:
            v = json.load(f)
        passes.append({"xlane": {k: v["xlane"][k] for k in SUMMARY_KEYS if k in v["xlane"]},
                       "before_it": {"valu_fp32_tflops": v["valu"]["fp32_tflops"], "lds_read_tbps": v["lds"]["read_tbps"],
                                     "l2_read_tbps": v["cache"]["l2_read_tbps"]}})
    defaults = {"waves_per_simd": ops.XLANE_WAVES_PER_SIMD, "rounds": ops.XLANE_ROUNDS, "rate_iters": ops.XLANE_RATE_ITERS}
    at_defaults = [r for r in runs if all(r[k] == v for k, v in defaults.items())]
    lowest = {k: min([r[k] for r in at_defaults] + [p["xlane"][k] for p in passes]) for k in RATES}
    out = {"what": WHAT,
           "units": {"dpp_tops": "10^12 lane-moves per second, v_mov_b32_dpp row_ror:1", "swap_tops": "alike, v_permlane32_swap_b32, 128 a wave instruction",
                     "bpermute_tops": "alike, ds_bpermute_b32", "swizzle_tops": "alike, ds_swizzle_b32"},
           "defaults": defaults,
           "lowest_run_at_defaults": {k: round(v, 2) for k, v in lowest.items()},
           "proposed_floors_25_percent_under_lowest": {k: round(0.75 * v, 1) for k, v in lowest.items()},
           "points": points, "fresh_process_passes": passes, "runs_at_defaults": [{k: r[k] for k in SUMMARY_KEYS if k in r} for r in at_defaults]}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(out["lowest_run_at_defaults"], out["proposed_floors_25_percent_under_lowest"])
    return 0


if __name__ == "__main__":
    sys.exit({"rates": rates, "pass": whole_pass, "summary": summary}[sys.argv[1]](*sys.argv[2:]))
