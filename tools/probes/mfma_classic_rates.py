"""fp16 / int8 / fp32 / fp64 MFMA rates of the diagnostics on the MI355X at the node agent's sizes:
each run of ops.mfma_classic() comes right after ops.mfma_lowp(), as in a pass.  Writes the runs as JSON.

    python3 tools/probes/mfma_classic_rates.py out.json
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from bacchus_gpu_controller_amd import ops  # noqa: E402


def main():
    path = sys.argv[1]
    runs = []
    for iters, n in ((2048, 3), (8192, 12), (16384, 3)):
        for _ in range(n):
            ops.mfma_lowp(0)
            t0 = time.time()
            r = ops.mfma_classic(0, 32, iters)
            r.update(iters=iters, wall_ms=round((time.time() - t0) * 1e3, 2))
            r.pop("bad_cu_keys")
            runs.append(r)
            print(iters, r["fp16_tflops"], r["int8_tops"], r["fp32_tflops"], r["fp64_tflops"], r["rate_ms"], r["elapsed_ms"],
                  r["wall_ms"], r["passed"], flush=True)
    with open(path, "w") as f:
        json.dump(runs, f, indent=1)
    return 0 if all(r["passed"] for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
