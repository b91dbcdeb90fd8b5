"""The fold of the diagnostics' per-key timing bins (native/gpu/hip/diag_fold.h: TimingFold) on its own, in a
stand-alone program that the host compiler builds from that header alone.

The program takes the ticks of one unit and one "ticks:count" pair per key, and prints the slowest key and, as
hexadecimal floats (so the comparison below is exact), the balance, the fastest, the slowest and every key's mean.

The recorded case feeds it the per-XCC numbers of the committed runs profiles/valu_diag/raw/pass_*.json.  Those hold
each XCC's count (xcc_wgs, xcc_waves) and mean in microseconds (xcc_us, xcc_wave_us), not the bins' tick sums; a sum
is a whole number of ticks of the 100 MHz clock, so it is mean * 100 * count rounded, and the case first checks that
the fold gives every recorded mean back exactly from those sums, then the recorded xcc_balance and slowest_xcc."""
import glob
import json
import os
import shutil
import subprocess

import pytest

from bacchus_gpu_controller_amd import REPO_ROOT

HIP_DIR = os.path.join(REPO_ROOT, "native", "gpu", "hip")
RUNS = sorted(glob.glob(os.path.join(REPO_ROOT, "profiles", "valu_diag", "raw", "pass_*.json")))
US = 100000 * 1e-3  # ticks of a microsecond, as cache.hip and mfma.hip compute it from the clock's kHz

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "diag_fold.h"

int main(int argc, char** argv) {
  const double ticks_per_unit = std::strtod(argv[1], nullptr);
  bgc_diag::TimingFold fold;
  std::printf("means");
  for (int k = 2; k < argc; ++k) {
    char* end = nullptr;
    const unsigned long long ticks = std::strtoull(argv[k], &end, 10);
    const unsigned n = static_cast<unsigned>(std::strtoul(end + 1, nullptr, 10));
    std::printf(" %a", fold.add(k - 2, ticks, n, ticks_per_unit));
  }
  std::printf("\n%d %a %a %a\n", fold.slowest_key, fold.balance(), fold.fastest, fold.slowest);
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("fold")
    src, out = str(d / "fold.cc"), str(d / "fold")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", HIP_DIR, src, "-o", out], check=True, timeout=120)
    return out


def fold(exe, ticks_per_unit, bins):
    """(slowest key, balance, fastest, slowest, means) of `bins`: one (ticks, count) per key"""
    p = subprocess.run([exe, float(ticks_per_unit).hex()] + ["%d:%d" % b for b in bins], capture_output=True, text=True, check=True, timeout=60)
    means, summary = p.stdout.splitlines()
    key, balance, fastest, slowest = summary.split()
    return int(key), float.fromhex(balance), float.fromhex(fastest), float.fromhex(slowest), [float.fromhex(m) for m in means.split()[1:]]


def mean(ticks, n, ticks_per_unit):
    return float(ticks) / n / ticks_per_unit


def test_no_key_ran(exe):
    assert fold(exe, 1.0, []) == (-1, 0.0, 0.0, 0.0, [])
    assert fold(exe, US, [(0, 0)] * 8) == (-1, 0.0, 0.0, 0.0, [0.0] * 8)


def test_one_key_is_balanced(exe):
    key, balance, fastest, slowest, means = fold(exe, 1.0, [(0, 0), (0, 0), (1234567, 32)])
    assert (key, balance) == (2, 1.0)
    assert fastest == slowest == means[2] == mean(1234567, 32, 1.0) and means[:2] == [0.0, 0.0]


def test_a_key_without_a_count_is_ignored(exe):
    # ticks without a count (key 0: low enough to be the fastest; key 2: high enough to be the slowest)
    key, balance, fastest, slowest, means = fold(exe, 1.0, [(1, 0), (3000, 3), (1 << 40, 0), (4400, 4)])
    assert (key, fastest, slowest) == (3, 1000.0, 1100.0)
    assert means == [0.0, 1000.0, 0.0, 1100.0] and balance == 1000.0 / 1100.0


@pytest.mark.parametrize("ticks_per_unit", [1.0, US])
def test_equal_means_keep_the_lower_key(exe, ticks_per_unit):
    # keys 1 and 3 are the slowest with the same mean from different sums; keys 0 and 2 the fastest
    key, balance, fastest, slowest, means = fold(exe, ticks_per_unit, [(500, 5), (2100, 7), (100, 1), (900, 3), (0, 0)])
    assert means[1] == means[3] and means[0] == means[2]
    assert key == 1 and slowest == means[1] and fastest == means[0]


@pytest.mark.parametrize("ticks_per_unit", [1.0, US, 99.99])
def test_balance_is_fastest_over_slowest_of_the_scaled_means(exe, ticks_per_unit):
    # sums and counts whose means are no round numbers, so the unit of the comparison shows in the last bit
    bins = [(10781924 + 7919 * k * k, 32 - (k % 3)) for k in range(8)] + [(0, 0), (3, 7)]
    want = [mean(t, n, ticks_per_unit) if n else 0.0 for t, n in bins]
    ran = [m for m, (_, n) in zip(want, bins) if n]
    key, balance, fastest, slowest, means = fold(exe, ticks_per_unit, bins)
    assert means == want
    assert (fastest, slowest) == (min(ran), max(ran))
    assert key == want.index(max(ran))
    assert balance == min(ran) / max(ran)


@pytest.mark.parametrize("section, counts, means_us, slowest_key",
                         [("cache", "xcc_wgs", "xcc_us", "slowest_xcc"), ("mfma", "xcc_waves", "xcc_wave_us", None)])
def test_recorded_runs_fold_to_their_recorded_balance(exe, section, counts, means_us, slowest_key):
    assert RUNS
    for path in RUNS:
        with open(path) as f:
            rec = json.load(f)[section]
        bins = [(round(us * US * n), n) for us, n in zip(rec[means_us], rec[counts])]
        key, balance, _, _, means = fold(exe, US, bins)
        assert means == rec[means_us], path  # the sums are the run's
        assert balance == rec["xcc_balance"], path
        if slowest_key:
            assert key == rec[slowest_key], path
