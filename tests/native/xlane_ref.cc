// A stand-alone program (its own main) over native/gpu/hip/xlane_ref.h, the cross-lane check's host reference: every
// DPP control at every lane, the gate at the bounds of its masks, the swaps, the permutes with every address, the
// swizzles, the scan, the EXEC mask, whole runs at the first and the last round count, and the rate phase's closed form
// at the bounds of its iterations.  tests/unit/test_native_xlane_ref.py builds it with AddressSanitizer and UBSan and
// runs it; it prints "ok".
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "gpu/hip/xlane_ref.h"

namespace ref = bgc_xlane;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                   \
    }                                                               \
  } while (0)

static void check_steps(const ref::Dpp* steps, int n) {
  for (int i = 0; i < n; ++i) {
    CHECK(steps[i].ctrl >= 0 && steps[i].ctrl <= ref::kRowBcast31 && steps[i].row_mask > 0 && steps[i].row_mask <= 0xf &&
          steps[i].bank_mask > 0 && steps[i].bank_mask <= 0xf);
    for (int l = 0; l < 64; ++l) {
      const int from = ref::dpp_source(steps[i].ctrl, l);
      CHECK(from >= -1 && from < 64);
    }
  }
}

int main() {
  // every control the encoding has, valid or not, at every lane: a source lane or -1
  for (int ctrl = 0; ctrl < 0x200; ++ctrl) {
    for (int l = 0; l < 64; ++l) {
      const int from = ref::dpp_source(ctrl, l);
      CHECK(from >= -1 && from < 64);
    }
  }
  check_steps(ref::RowSteps::steps, ref::RowSteps::kCount);
  check_steps(ref::WaveSteps::steps, ref::WaveSteps::kCount);
  check_steps(ref::MaskSteps::steps, ref::MaskSteps::kCount);
  check_steps(ref::ScanSteps::steps, ref::ScanSteps::kCount);
  const ref::Dpp singles[] = {ref::kAluAdd, ref::kAluMin, ref::kExecKeep, ref::kExecZero, ref::kRateDpp};
  check_steps(singles, 5);
  CHECK(ref::dpp_source(ref::row_shr(1), 0) == -1 && ref::dpp_source(ref::row_shr(1), 16) == -1 && ref::dpp_source(ref::row_shr(1), 63) == 62);
  CHECK(ref::dpp_source(ref::row_shl(15), 0) == 15 && ref::dpp_source(ref::row_shl(15), 1) == -1);
  CHECK(ref::dpp_source(ref::kWaveShl1, 63) == -1 && ref::dpp_source(ref::kWaveRol1, 63) == 0 && ref::dpp_source(ref::kWaveRor1, 0) == 63);

  // the gate: empty and full masks, every lane of EXEC alone
  uint32_t src[64], old[64], out[64];
  for (int l = 0; l < 64; ++l) {
    src[l] = 0x100u + static_cast<uint32_t>(l);
    old[l] = 0x200u + static_cast<uint32_t>(l);
  }
  for (int l = 0; l < 64; ++l) {
    for (int i = 0; i < 64; ++i) out[i] = old[i];
    ref::dpp_mov({ref::kWaveRor1, 0xf, 0xf, 1}, 1ULL << l, src, out);
    for (int i = 0; i < 64; ++i) CHECK(out[i] == (i == l ? 0u : old[i]));  // its source lane is disabled
  }
  for (int i = 0; i < 64; ++i) out[i] = old[i];
  ref::dpp_mov({ref::row_ror(1), 0x0, 0x0, 1}, ref::kAllLanes, src, out);
  for (int i = 0; i < 64; ++i) CHECK(out[i] == old[i]);
  ref::dpp_mov({ref::row_ror(1), 0xf, 0xf, 0}, ref::kAllLanes, src, out);
  for (int i = 0; i < 64; ++i) CHECK(out[i] == src[(i & ~15) | ((i - 1) & 15)]);

  // swaps are involutions that keep every value
  for (int width : {16, 32}) {
    uint32_t a[64], b[64];
    for (int l = 0; l < 64; ++l) {
      a[l] = src[l];
      b[l] = old[l];
    }
    ref::permlane_swap(width, a, b);
    CHECK(a[width] == old[0] && b[0] == src[width] && a[0] == src[0] && b[63] == old[63]);
    ref::permlane_swap(width, a, b);
    for (int l = 0; l < 64; ++l) CHECK(a[l] == src[l] && b[l] == old[l]);
  }

  // permutes: every address a lane can give, masked or not, and the all-ones address
  uint32_t addr[64];
  for (uint32_t base : {0u, 0xffffff00u, 0xfffffffcu - 63 * 4}) {
    for (int l = 0; l < 64; ++l) addr[l] = base + 4u * static_cast<uint32_t>(63 - l) + 3u;
    ref::ds_bpermute(ref::kAllLanes, addr, src, out);
    for (int l = 0; l < 64; ++l) CHECK(out[l] == src[(addr[l] >> 2) & 63]);
    ref::ds_permute(addr, src, out);
    for (int l = 0; l < 64; ++l) CHECK(out[(addr[l] >> 2) & 63] == src[l]);
  }
  for (int l = 0; l < 64; ++l) addr[l] = 0xffffffffu;
  ref::ds_bpermute(1ULL << 63, addr, src, out);
  CHECK(out[63] == src[63]);
  ref::ds_bpermute(1ULL, addr, src, out);
  CHECK(out[0] == 0);  // lane 63 is inactive
  for (int offset : {0, 0x7fff, 0x8000, 0x80ff, 0xffff, ref::kSwizzle[0], ref::kSwizzle[1], ref::kSwizzle[2], ref::kRateSwizzle}) {
    for (int l = 0; l < 64; ++l) {
      const int from = ref::swizzle_source(offset, l);
      CHECK(from >= 0 && from < 64 && (from & 32) == (l & 32));
    }
  }
  CHECK(ref::first_lane(1ULL << 63) == 63 && ref::first_lane(ref::kAllLanes) == 0 && ref::mbcnt(ref::kAllLanes, 63) == 63 &&
        ref::mbcnt(ref::kAllLanes, 0) == 0 && ref::mbcnt(1ULL << 63, 63) == 0);

  // whole runs: the first and the last round count, three seeds; the addresses and masks of every round
  for (uint32_t seed : {0x5eedu, 0u, 0xffffffffu}) {
    for (int rounds : {1, 64}) {
      std::vector<uint32_t> raw(static_cast<size_t>(rounds) * ref::kRoundWords * 64), digests(ref::kClasses * 64);
      ref::expected(seed, rounds, raw.data(), digests.data());
      ref::expected(seed, rounds, nullptr, nullptr);
      std::vector<uint32_t> again(digests.size());
      ref::expected(seed, rounds, nullptr, again.data());
      CHECK(again == digests);
      for (int r = 0; r < rounds; ++r) {
        const uint32_t* scan = raw.data() + (static_cast<size_t>(r) * ref::kRoundWords + ref::word_base(BGC_XLANE_ALU) + 2) * 64;
        uint32_t sum = 0;
        for (int l = 0; l < 64; ++l) {
          sum += ref::operand(seed, BGC_XLANE_ALU, r, 2, l);
          CHECK(scan[l] == sum);
        }
        const uint64_t m = ref::exec_mask(seed, r);
        CHECK(m != 0 && m != ref::kAllLanes);
        std::set<uint32_t> targets;
        for (int l = 0; l < 64; ++l) {
          CHECK(ref::rotate_addr(seed, r, l) <= 252 && ref::scatter_addr(seed, r, l) <= 252 && ref::rotate_addr(seed, r, l) != 4u * l);
          targets.insert(ref::scatter_addr(seed, r, l));
        }
        CHECK(targets.size() == 64);
        CHECK(ref::readlane_select(seed, r) >= 0 && ref::readlane_select(seed, r) < 64 && ref::writelane_select(seed, r) >= 0 &&
              ref::writelane_select(seed, r) < 64);
      }
    }
  }

  // the rate phase: every class at the bounds of the iterations; a step is a permutation, and the closed form equals
  // the steps taken one by one
  for (int cls = 0; cls < ref::kRateClasses; ++cls) {
    std::set<int> sources;
    for (int s = 0; s < ref::kSlots; ++s) {
      const int from = ref::rate_source(cls, s);
      CHECK(from >= 0 && from < ref::kSlots);
      sources.insert(from);
    }
    CHECK(static_cast<int>(sources.size()) == ref::kSlots);
    uint32_t ends[64], state[ref::kSlots], next[ref::kSlots];
    for (int s = 0; s < ref::kSlots; ++s) state[s] = ref::rate_fill(0x5eed, s % 64, s / 64);
    for (int n = 1; n <= 37; ++n) {
      for (int s = 0; s < ref::kSlots; ++s) next[s] = state[ref::rate_source(cls, s)];
      for (int s = 0; s < ref::kSlots; ++s) state[s] = next[s];
      ref::rate_expected(cls, 0x5eed, n, ends);
      for (int l = 0; l < 64; ++l) {
        uint32_t d = ref::rate_digest_start(cls);
        for (int c = 0; c < ref::kChains; ++c) d = ref::mix32(d ^ state[c * 64 + l]);
        CHECK(ends[l] == d);
      }
    }
    ref::rate_expected(cls, 0xffffffffu, 1 << 16, ends);
    ref::rate_expected(cls, 0, 65535, ends);
  }
  if (failures == 0) std::puts("ok");
  return failures != 0;
}
