"""LDS read rate of the diagnostics on the MI355X at the node agent's sizes: each run of ops.lds()
comes right after ops.mfma(), so the clocks are as in a pass.  Writes the runs as JSON.

    python3 tools/probes/lds_rate_probe.py 512 out.json

The first argument only labels the runs.  To measure the other workgroup size of lds_rate, build
the library with -DBGC_LDS_RATE_THREADS=256 and point BGC_GPU_DIAG_LIB at it.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from bacchus_gpu_controller_amd import ops  # noqa: E402


def main():
    threads, path = int(sys.argv[1]), sys.argv[2]
    runs = []
    for iters, n in ((2048, 3), (8192, 12), (16384, 3)):
        for _ in range(n):
            m = ops.mfma(0, 16, 2048)
            t0 = time.time()
            r = ops.lds(0, 4, iters)
            r.update(rate_iters=iters, threads=threads, wall_ms=round((time.time() - t0) * 1e3, 2), mfma_tflops=m["tflops"])
            r.pop("bad_cu_keys")
            runs.append(r)
            print(threads, iters, r["read_tbps"], r["cus_seen"], r["cus"], r["cu_balance"], r["elapsed_ms"], r["passed"], flush=True)
    with open(path, "w") as f:
        json.dump(runs, f, indent=1)
    return 0 if all(r["passed"] for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
