"""Vector-ALU rates and transcendental accuracy of the diagnostics on the MI355X.  Writes the runs as JSON.

    python3 tools/probes/valu_rate_probe.py rates out.json     # 12 runs back to back per point
    python3 tools/probes/valu_rate_probe.py pass out.json      # one whole pass; run it in a fresh process
    python3 tools/probes/valu_rate_probe.py ulps out.json      # the transcendentals against numpy float64
    python3 tools/probes/valu_rate_probe.py summary rates.json pass1.json ... out.json   # needs no GPU

* rates: ops.valu() at 1, 2, 4 and 8 waves per SIMD and 1024, 4096 and 16384 rate iterations, each run
  right after ops.mfma(), so the clocks are as in a pass; then 12 runs at ops.valu()'s defaults.  Every
  run records the five rates, the time of each timed launch and of all kernels together, and the wall
  time of the call, which is what the defaults in ops are sized from.
* pass: hbm, mfma, mfma_lowp, mfma_classic, lds, cache and valu at their defaults, once, as a node
  agent's pass orders them: the rates that a floor has to hold against.
* ulps: the raw v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32 and v_sqrt_f32 results of wave 0 at 64 rounds
  for seed 0x5eed and 16 others (69632 values per instruction): the largest error in units of the last
  place of the fp32 result, which BGC_VALU_*_ULPS in gpu_diag.h are derived from.
* summary: the `rates` file and the `pass` files as one record: the range of every rate, time and balance per
  point, the runs at the defaults, the lowest run of each rate there and the floor 25 % under it.
  profiles/valu_diag/rates.json is this, made from the files in profiles/valu_diag/raw/.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from bacchus_gpu_controller_amd import ops  # noqa: E402

RUNS = 12
RATES = ("fp32_tflops", "fp16_tflops", "fp64_tflops", "int32_tops", "trans_tips")
SEEDS = [0x5EED] + [(0x9E3779B9 * (i + 1)) & 0xFFFFFFFF for i in range(16)]
TRANS_BASE = 35  # the first transcendental word of a round's 40
INSTRUCTIONS = ("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32")


def one(label, **args):
    m = ops.mfma(0, 16, 2048)
    t0 = time.time()
    r = ops.valu(0, **args)
    r.update(label=label, wall_ms=round((time.time() - t0) * 1e3, 2), mfma_tflops=m["tflops"], **args)
    return r


def rates(path):
    runs = []
    points = [(wps, iters) for wps in (1, 2, 4, 8) for iters in (1024, 4096, 16384)]
    points.append((ops.VALU_WAVES_PER_SIMD, ops.VALU_RATE_ITERS))
    for i, (wps, iters) in enumerate(points):
        label = "defaults" if i == len(points) - 1 else "sweep"
        for _ in range(RUNS):
            r = one(label, waves_per_simd=wps, rounds=ops.VALU_ROUNDS, rate_iters=iters)
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
                     ("valu", lambda: ops.valu(0))):
        t0 = time.time()
        out[name] = fn()
        out[name]["wall_ms"] = round((time.time() - t0) * 1e3, 2)
    v = out["valu"]
    print("pass", [round(v[k], 2) for k in RATES], [round(ms, 3) for ms in v["rate_ms"]], round(v["elapsed_ms"], 3), v["wall_ms"], v["passed"],
          flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    return 0 if all(r["passed"] for r in out.values()) else 1


SUMMARY_KEYS = ("label", "waves_per_simd", "rounds", "rate_iters") + RATES + (
    "rate_ms", "elapsed_ms", "wall_ms", "cus_seen", "simds_seen", "cu_balance", "slowest_cu_key", "values_checked", "mismatches", "consensus_ok",
    "trans_out_of_bound", "rate_ok", "passed", "mfma_tflops")
WHAT_RATES = ("tools/probes/valu_rate_probe.py on one MI355X (gfx950, 256 CUs): `rates` (12 runs back to back per point, each right after "
              "ops.mfma) and `pass` (hbm, mfma, mfma_lowp, mfma_classic, lds, cache, valu at their defaults in a fresh process), joined by `summary`")
WHAT_ULPS = ("tools/probes/valu_rate_probe.py ulps on one MI355X: the largest error of each transcendental instruction against numpy float64, in "
             "units of the last place of the fp32 result, over seed 0x5eed and 16 others at 64 rounds; bound = ceil(max) + 1 (the host libm's own "
             "error), as BGC_VALU_*_ULPS in gpu_diag.h")


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
        passes.append({"valu": {k: v["valu"][k] for k in SUMMARY_KEYS if k in v["valu"]},
                       "before_it": {"mfma_classic_fp32_tflops": v["mfma_classic"]["fp32_tflops"], "lds_read_tbps": v["lds"]["read_tbps"],
                                     "l2_read_tbps": v["cache"]["l2_read_tbps"]}})
    defaults = {"waves_per_simd": ops.VALU_WAVES_PER_SIMD, "rounds": ops.VALU_ROUNDS, "rate_iters": ops.VALU_RATE_ITERS}
    at_defaults = [r for r in runs if all(r[k] == v for k, v in defaults.items())]
    lowest = {k: min([r[k] for r in at_defaults] + [p["valu"][k] for p in passes]) for k in RATES}
    out = {"what": WHAT_RATES,
           "units": {"fp32_tflops": "TFLOP/s, v_pk_fma_f32, an FMA counts 2", "fp16_tflops": "TFLOP/s, v_pk_fma_f16", "fp64_tflops": "TFLOP/s, v_fma_f64",
                     "int32_tops": "TOP/s, v_mad_u32_u24, a mad counts 2", "trans_tips": "10^12 v_exp_f32 per second"},
           "known_in_advance": {"fp32_vector_peak_tflops": 157.3}, "defaults": defaults,
           "lowest_run_at_defaults": {k: round(v, 2) for k, v in lowest.items()},
           "proposed_floors_25_percent_under_lowest": {k: round(0.75 * v, 1) for k, v in lowest.items()},
           "points": points, "fresh_process_passes": passes, "runs_at_defaults": [{k: r[k] for k in SUMMARY_KEYS if k in r} for r in at_defaults]}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(out["lowest_run_at_defaults"], out["proposed_floors_25_percent_under_lowest"])
    return 0


def trans_reference(operands):
    x = [v.astype(np.float64) for v in operands]
    return [np.exp2(x[0]), np.log2(x[1]), 1.0 / x[2], 1.0 / np.sqrt(x[3]), np.sqrt(x[4])]


def trans_operands(seed, r):
    """gpu_diag.h, "Vector ALU": the operands of the five transcendental words of round r, 64 lanes each"""
    def mix32(x):
        x = np.array(x, dtype=np.uint32)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
        return x

    def f32(h, emin=-8, mask=15):
        return (h & np.uint32(0x807FFFFF)) | ((np.uint32(127 + emin) + ((h >> np.uint32(23)) & np.uint32(mask))) << np.uint32(23))

    lanes = np.arange(64, dtype=np.uint32)
    w = [mix32(np.uint32(seed) ^ mix32(np.uint32(6 << 24 | r << 16 | k << 8) | lanes)) for k in range(5)]
    t = ((w[1] >> np.uint32(23)) & np.uint32(7)).astype(np.int64)
    log_in = (w[1] & np.uint32(0x007FFFFF)) | ((127 + np.where(t < 4, t - 5, t - 3)).astype(np.uint32) << np.uint32(23))
    pos = np.uint32(0x7FFFFFFF)
    return [f32(w[0], -2, 7).view(np.float32), log_in.view(np.float32), f32(w[2]).view(np.float32), (f32(w[3]) & pos).view(np.float32),
            (f32(w[4]) & pos).view(np.float32)]


def ulps_off(raw, want):
    """|got - want| in units of the last place of want as an fp32 number"""
    got = raw.view(np.float32).astype(np.float64)
    return np.abs(got - want) / np.exp2(np.floor(np.log2(np.abs(want))) - 23)


def ulps(path):
    worst = np.zeros(5)
    by_seed = []
    for seed in SEEDS:
        r, wave = ops.valu_data(0, waves_per_simd=1, rounds=64, rate_iters=16, seed=seed)
        mine = np.zeros(5)
        for rnd in range(64):
            for op, want in enumerate(trans_reference(trans_operands(seed, rnd))):
                mine[op] = max(mine[op], ulps_off(wave["raw"][rnd, TRANS_BASE + op], want).max())
        worst = np.maximum(worst, mine)
        by_seed.append({"seed": seed, "max_ulps": mine.tolist(), "trans_out_of_bound": r["trans_out_of_bound"], "consensus_ok": r["consensus_ok"],
                        "passed": r["passed"]})
        print(f"{seed:#010x}", [round(float(u), 4) for u in mine], r["trans_out_of_bound"], r["passed"], flush=True)
    out = {"what": WHAT_ULPS, "instructions": INSTRUCTIONS, "values_per_instruction": len(SEEDS) * 64 * 64, "max_ulps": worst.tolist(),
           "bound_ulps": [float(np.ceil(u) + 1) for u in worst], "bounds_in_library": list(ops.valu_trans_ulps()), "seeds": by_seed}
    print("max", out["max_ulps"], "bound", out["bound_ulps"], "library", out["bounds_in_library"], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit({"rates": rates, "pass": whole_pass, "ulps": ulps, "summary": summary}[sys.argv[1]](*sys.argv[2:]))
