#!/usr/bin/env python3
"""Driver contract entry point: `python bench.py --gpus N --steps K --warmup W`.

Runs the headline UserBootstrap churn benchmark (see
bacchus_gpu_controller_amd/bench/harness.py) and prints one JSON line on rank 0.
Under torchrun each rank drives one GPU; the native binaries are built in-tree first.

A plain run times the headline phase alone.  Two options belong to this file, every other
argument goes to the harness:

  --full              also run the harness's secondary measurements (isolated, tuned and
                      HTTP/1.1 phases, reference-controller and write-latency arms, traced
                      open-loop windows, RCCL/xGMI probe on N>1 GPUs), each under its own switch
  --dump-outputs DIR  after the timed steps, write what the last one produced as
                      DIR/<name>.npy (see _Dump)

Both work through the harness's command line and the native module's ChurnDriver only, so
this file can drive another build of the package and the two can be compared.
"""
import argparse
import glob
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# what a run without --full leaves out
PLAIN = ["--no-isolated-phase", "--no-tuned-phase", "--no-http1-phase", "--no-reference-arms", "--no-trace-windows",
         "--latency-rates", "", "--xgmi-probe-mb", ""]


def _artefacts_present():
    pkg = os.path.join(ROOT, "bacchus_gpu_controller_amd")
    return (os.path.exists(os.path.join(ROOT, "bin", "kube-lite")) and glob.glob(os.path.join(pkg, "_native*.so"))
            and os.path.exists(os.path.join(pkg, "libbgc_gpu_diag.so")))


def _ensure_built():
    # Build once (rank 0 / single process); other ranks wait for the artefacts.
    rank = int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0")))
    marker = os.path.join(ROOT, "bin", "kube-lite")
    build_dir = os.path.join(ROOT, "build")
    if _artefacts_present() and not os.access(build_dir if os.path.isdir(build_dir) else ROOT, os.W_OK):
        # A built tree whose build directory this user may not write is run as it is, like an
        # installed package: ninja could not even take its lock or write its log there, and
        # keeping such a tree current is up to whoever owns it (build()).
        return
    if rank == 0:
        from bacchus_gpu_controller_amd.utils.build import ensure_built

        # stdout carries exactly one JSON line: build chatter (ninja/hipcc are child
        # processes writing to fd 1) goes to stderr
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            ensure_built()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)
    else:
        import time

        for _ in range(600):
            if os.path.exists(marker):
                break
            time.sleep(0.5)


QUOTA_KEYS = ("requests.cpu", "requests.memory", "limits.cpu", "limits.memory", "requests.amd.com/gpu",
              "requests.storage", "requests.amd.com/gpu-partition")
_QUANTITY_SUFFIX = {"": 1.0, "m": 1e-3, "k": 1e3, "M": 1e6, "G": 1e9, "T": 1e12,
                    "Ki": 2.0 ** 10, "Mi": 2.0 ** 20, "Gi": 2.0 ** 30, "Ti": 2.0 ** 40}
_HEADLINE_NAME = re.compile(r"^r\d+-m(\d+)-u\d+$")  # harness._names() of the headline phase "m"


def _quantity(text):
    """A Kubernetes quantity ("8", "64Gi", "500m") as a float; NaN when absent or malformed."""
    text = str(text if text is not None else "").strip()
    digits = text.rstrip("KMGTkmi")
    try:
        return float(digits) * _QUANTITY_SUFFIX[text[len(digits):]]
    except (ValueError, KeyError):
        return float("nan")


class _Dump:
    """--dump-outputs: the results of the headline phase's last timed step, ranks concatenated
    in rank order.  Tenant names and sheet rows depend on the arguments alone, so two builds
    run with the same arguments can be compared array for array.

    round_counts     float64 [ranks * rounds, 3]  Ready, failed and timed-out tenants of each round
    tenant_children  float32 [ranks * batch, 3]   last round: Namespace, ResourceQuota, RoleBinding exist
    tenant_quota     float64 [ranks * batch, 7]   last round: the quota's spec.hard over QUOTA_KEYS

    The harness drives every step through the native module's ChurnDriver, so the driver is
    wrapped: each round's counts are kept as step_with_delete() returns them, and when the
    harness removes the last round's tenants (remove(), after its timed region) their
    children are read from the API server first."""

    def __init__(self, path):
        self.path, self.args, self.rounds, self.written = path, None, [], False

    def install(self):
        import bacchus_gpu_controller_amd as pkg
        from bacchus_gpu_controller_amd.bench import harness

        dump, native, run = self, pkg.native, harness.run

        class Driver:
            def __init__(self, server, token, *a, **kw):
                self._d = native().ChurnDriver(server, token, *a, **kw)
                self._api = (server, token, kw.get("ca_pem", ""))

            def __getattr__(self, name):
                return getattr(self._d, name)

            def step_with_delete(self, names, previous, timeout):
                res = self._d.step_with_delete(names, previous, timeout)
                m = _HEADLINE_NAME.match(names[0]) if names else None
                if m and int(m.group(1)) // dump.args.rounds == dump.args.warmup + dump.args.steps - 1:
                    dump.rounds.append(res)  # the last timed step; parsed in write(), outside the timed region
                return res

            def remove(self, names):
                if names and _HEADLINE_NAME.match(names[0]) and not dump.written:
                    dump.write(self._api, list(names))
                return self._d.remove(names)

        class Native:
            ChurnDriver = Driver

            def __getattr__(self, name):
                return getattr(native(), name)

        def traced_run(args):
            dump.args = args
            return run(args)

        proxy = Native()
        pkg.native = lambda: proxy
        harness.run = traced_run

    def write(self, api, names):
        import numpy as np

        from bacchus_gpu_controller_amd.testing.kubeapi import KubeApi

        results = [json.loads(res) for res in self.rounds]
        counts = [[r["ready"], r["failed"], r["timeouts"]] for r in results]
        server, token, ca_pem = api
        with tempfile.NamedTemporaryFile("w", suffix=".crt") as ca:
            ca.write(ca_pem)
            ca.flush()
            kube = KubeApi(server, token, verify=ca.name if ca_pem else True)
            children, quota = [], []
            for n in names:
                ns = kube.get_or_none("namespaces", n)
                rq = kube.get_or_none("resourcequotas", n, n)
                rb = kube.get_or_none("rolebindings", n, n)
                children.append([float(o is not None) for o in (ns, rq, rb)])
                hard = ((rq or {}).get("spec") or {}).get("hard") or {}
                quota.append([_quantity(hard.get(k)) for k in QUOTA_KEYS])
        per_rank = [{"round_counts": counts, "tenant_children": children, "tenant_quota": quota}]
        rank = 0
        try:
            import torch.distributed as dist

            if dist.is_available() and dist.is_initialized():
                rank, mine = dist.get_rank(), per_rank[0]
                per_rank = [None] * dist.get_world_size()
                dist.all_gather_object(per_rank, mine)
        except ImportError:
            pass
        self.written = True
        if rank != 0:
            return
        os.makedirs(self.path, exist_ok=True)
        cat = lambda key: [row for p in per_rank for row in p[key]]  # noqa: E731
        for name, dtype, width in (("round_counts", np.float64, 3), ("tenant_children", np.float32, 3),
                                   ("tenant_quota", np.float64, len(QUOTA_KEYS))):
            np.save(os.path.join(self.path, name + ".npy"), np.asarray(cat(name), dtype=dtype).reshape(-1, width))


def main(argv):
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--dump-outputs", default="", metavar="DIR")
    own, rest = ap.parse_known_args(argv)
    from bacchus_gpu_controller_amd.bench import harness

    if "-h" in rest or "--help" in rest:
        print(__doc__)
        return harness.main(["--help"])  # argparse prints the harness's options and exits: no build
    _ensure_built()

    dump = None
    if own.dump_outputs:
        dump = _Dump(own.dump_outputs)
        dump.install()
    # explicit arguments come last and so still win over PLAIN
    rc = harness.main(rest if own.full else PLAIN + rest)
    if dump is not None and not dump.written:
        print("bench.py: --dump-outputs wrote nothing: the headline phase never reached its end", file=sys.stderr)
        return 1
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
