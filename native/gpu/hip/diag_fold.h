// The fold of a rate launch's per-key timing bins (key: a CU or an XCC) into the fastest and the slowest key's mean
// and their balance.  No HIP dependency: diag_common.h includes it for lds.hip, cache.hip, valu.hip and mfma.hip, and
// a plain C++17 program can include it alone (tests/unit/test_diag_fold.py).
#pragma once

namespace bgc_diag __attribute__((visibility("hidden"))) {

// add() every key in ascending order.  The comparison is in the unit that `ticks_per_unit` sets (1.0: ticks; the
// constant clock's MHz: microseconds), so of two keys whose means are equal there the lower one stays the slowest.
struct TimingFold {
  double fastest = 0, slowest = 0;  // means, in that unit; 0 while no key ran
  int slowest_key = -1;

  // A key whose `n` workgroups or waves took `ticks` in all: its mean, or 0.0 for a key on which none ran.
  double add(int key, unsigned long long ticks, unsigned n, double ticks_per_unit) {
    if (!n) return 0.0;
    const double mean = static_cast<double>(ticks) / n / ticks_per_unit;
    fastest = fastest == 0 ? mean : mean < fastest ? mean : fastest;
    if (mean > slowest) {
      slowest = mean;
      slowest_key = key;
    }
    return mean;
  }

  // fastest / slowest: 1.0 when every key took the same time, 0.0 when none ran
  double balance() const { return slowest > 0 ? fastest / slowest : 0.0; }
};

}  // namespace bgc_diag
