"""L2 and Infinity-Cache read rates of the diagnostics on the MI355X: each run of ops.cache() comes
right after ops.mfma(), so the clocks are as in a pass.  Writes the runs as JSON.

    python3 tools/probes/cache_rate_probe.py LABEL out.json [l2|ic|all]

* L2: regions of 32, 64, 96 and 128 KiB with the Infinity-Cache phase off, 12 runs each.
* Infinity Cache: buffers of 32, 64, 128, 192, 256 and 512 MiB, 12 runs each, every point reading
  about 16 GiB in its timed launch, and the read rate of ops.hbm(nbytes=1 << 30) in the same process.
* The whole run at ops.cache()'s defaults, 12 times.
* Each run also records the time of its timed launch (bytes / rate), which is what the default sweep
  counts in ops are sized from.

LABEL only labels the runs.  To measure the other variants of the rate kernels, build the library
with -DBGC_L2_RATE_NT=0 (plain instead of nontemporal L2 loads), -DBGC_IC_RATE_NT=1 (nontemporal
instead of plain Infinity-Cache loads) or -DBGC_L2_RATE_THREADS=512 and point BGC_GPU_DIAG_LIB at it.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from bacchus_gpu_controller_amd import ops  # noqa: E402

KIB, MIB = 1 << 10, 1 << 20
RUNS = 12
L2_SWEEPS = ops.L2_SWEEPS
IC_READ_BYTES = ops.IC_BYTES * ops.IC_SWEEPS  # 16 GiB


def one(label, **args):
    m = ops.mfma(0, 16, 2048)
    t0 = time.time()
    r = ops.cache(0, **args)
    r.update(label=label, l2_sweeps=args["l2_sweeps"], ic_sweeps=args["ic_sweeps"], wall_ms=round((time.time() - t0) * 1e3, 2),
             mfma_tflops=m["tflops"])
    r["l2_rate_ms"] = r["cus"] * args["l2_sweeps"] * r["region_bytes"] / r["l2_read_tbps"] / 1e9
    if r["ic_bytes"]:
        r["ic_rate_ms"] = r["ic_bytes"] * args["ic_sweeps"] / r["ic_read_tbps"] / 1e9
    return r


def main():
    label, path = sys.argv[1], sys.argv[2]
    which = sys.argv[3] if len(sys.argv) > 3 else "all"
    runs, hbm = [], []
    if which in ("l2", "all"):
        for region in (32 * KIB, 64 * KIB, 96 * KIB, 128 * KIB):
            for _ in range(RUNS):
                r = one(label, rounds=4, region_bytes=region, l2_sweeps=L2_SWEEPS, ic_bytes=0, ic_sweeps=1)
                runs.append(r)
                print(label, "l2", region // KIB, round(r["l2_read_tbps"], 2), round(r["l2_rate_ms"], 3), r["xcc_balance"], r["xcc_wgs"],
                      r["passed"], flush=True)
    if which == "all":  # the run as ops.cache() does it by default
        for _ in range(RUNS):
            r = one(label + " defaults", rounds=4, region_bytes=ops.L2_REGION_BYTES, l2_sweeps=ops.L2_SWEEPS, ic_bytes=ops.IC_BYTES,
                    ic_sweeps=ops.IC_SWEEPS)
            runs.append(r)
            print(label, "defaults", round(r["l2_read_tbps"], 2), round(r["l2_rate_ms"], 3), round(r["ic_read_tbps"], 2),
                  round(r["ic_rate_ms"], 3), r["elapsed_ms"], r["wall_ms"], r["passed"], flush=True)
    if which in ("ic", "all"):
        for mib in (32, 64, 128, 192, 256, 512):
            for _ in range(RUNS):
                r = one(label, rounds=1, region_bytes=32 * KIB, l2_sweeps=16, ic_bytes=mib * MIB, ic_sweeps=max(1, IC_READ_BYTES // (mib * MIB)))
                runs.append(r)
                print(label, "ic", mib, round(r["ic_read_tbps"], 2), round(r["ic_rate_ms"], 3), r["passed"], flush=True)
        for _ in range(4):
            ops.mfma(0, 16, 2048)
            h = ops.hbm(0, nbytes=1 << 30)
            hbm.append({k: h[k] for k in ("bytes", "iters", "read_gbps", "write_gbps", "copy_gbps", "passed")})
            print(label, "hbm", h["read_gbps"], flush=True)
    with open(path, "w") as f:
        json.dump({"label": label, "runs": runs, "hbm": hbm}, f, indent=1)
    return 0 if all(r["passed"] for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
