// A stand-alone program (its own main) over native/gpu/hip/regfile_ref.h, the register-file check's host reference:
// the layouts, the pattern's conditions, the expected contents of every phase, a plant at every slot in every phase
// that holds it, its journey round the ring, and the bounds of every list.  tests/unit/test_native_regfile_ref.py
// builds it with AddressSanitizer and UBSan and runs it; it prints "ok".
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "gpu/hip/regfile_ref.h"

namespace ref = bgc_regfile;

struct Plant {
  int wave, phase, slot, lane;
  uint32_t xor_mask;
};

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                   \
    }                                                               \
  } while (0)

int main() {
  // layouts: each leaves out its own eight, together they march all 512; the ring is 504 registers, each once
  for (int reg = 0; reg < ref::kRegs; ++reg) CHECK(!ref::is_temp(0, reg) || !ref::is_temp(1, reg));
  for (int layout = 0; layout < 2; ++layout) {
    int marched = 0;
    for (int reg = 0; reg < ref::kRegs; ++reg) marched += !ref::is_temp(layout, reg);
    CHECK(marched == ref::marched_regs(layout));
  }
  std::set<int> ring;
  for (int i = 0; i < ref::kRing; ++i) {
    const int reg = ref::ring_reg(i);
    CHECK(reg >= 0 && reg < ref::kRegs && !ref::is_temp(0, reg) && ref::ring_index(reg) == i);
    ring.insert(reg);
  }
  CHECK(static_cast<int>(ring.size()) == ref::kRing && ref::kRing >= 496);
  for (int sweeps : {1, 2, ref::kRing - 1, ref::kRing, ref::kRing + 1, 4096, 65536}) {
    for (int reg : {ref::kRingFirst, 255, 256, 511}) {
      CHECK(ref::came_from(ref::travelled_to(reg, sweeps), sweeps) == reg);
      CHECK(ring.count(ref::travelled_to(reg, sweeps)) == 1);
    }
  }
  CHECK(ref::travelled_to(ref::kRingFirst, 1) == 511 && ref::travelled_to(511, 1) == 510 && ref::came_from(511, 1) == ref::kRingFirst);

  // the pattern: inverse passes, distinct registers of a lane, distinct lanes of a register
  std::vector<uint32_t> words(ref::kWords), other(ref::kWords);
  for (uint32_t seed : {0x5eedu, 0u, 0xffffffffu}) {
    const uint32_t ws = ref::wave_seed(seed, 5);
    for (int lane = 0; lane < ref::kLanes; ++lane) {
      std::set<uint32_t> seen;
      for (int reg = 0; reg < ref::kRegs; ++reg) {
        CHECK((ref::pattern(ws, reg, lane, 0) ^ ref::pattern(ws, reg, lane, 1)) == ~0u);
        seen.insert(ref::pattern(ws, reg, lane, 0));
      }
      CHECK(seen.size() == static_cast<size_t>(ref::kRegs));
    }
    for (int reg = 0; reg < ref::kRegs; ++reg) {
      std::set<uint32_t> seen;
      for (int lane = 0; lane < ref::kLanes; ++lane) seen.insert(ref::pattern(ws, reg, lane, 0));
      CHECK(seen.size() == static_cast<size_t>(ref::kLanes));
    }
    // expected(): every phase, without plants
    for (int phase = 0; phase < ref::kPhases; ++phase) {
      ref::expected<Plant>(seed, 5, phase, 7, nullptr, 0, words.data());
      for (int reg = 0; reg < ref::kRegs; ++reg) {
        const int from = phase == ref::kPhaseRotate && reg >= ref::kRingFirst ? ref::came_from(reg, 7) : reg;
        const uint32_t want = ref::phase_holds(phase, reg) ? ref::pattern(ws, from, 63, phase == ref::kPhaseRotate ? 0 : phase & 1) : 0u;
        CHECK(words[static_cast<size_t>(reg) * ref::kLanes + 63] == want);
      }
    }
  }

  // a plant at every slot, in every phase that holds it: one word differs, where the header says
  int temps_with_a_slot[2] = {0, 0};
  for (int slot = 0; slot < ref::kPlantSlots; ++slot) {
    const int reg = ref::kPlantRegs[slot];
    CHECK(reg >= 0 && reg < ref::kRegs);
    for (int layout = 0; layout < 2; ++layout) temps_with_a_slot[layout] += ref::is_temp(layout, reg);
    for (int phase = 0; phase < ref::kPhases; ++phase) {
      const Plant p{5, phase, slot, (slot * 9) % ref::kLanes, 0x80000001u};
      CHECK(ref::plant_ok(p) == ref::phase_holds(phase, reg));
      if (!ref::plant_ok(p)) continue;
      for (int sweeps : {1, ref::kRing - 1, ref::kRing, ref::kRing + 1}) {
        ref::expected<Plant>(0x5eed, 5, phase, sweeps, nullptr, 0, words.data());
        ref::expected(0x5eed, 5, phase, sweeps, &p, 1, other.data());
        const int at = phase == ref::kPhaseRotate ? ref::travelled_to(reg, sweeps) : reg;
        int differ = 0;
        for (int w = 0; w < ref::kWords; ++w) differ += words[static_cast<size_t>(w)] != other[static_cast<size_t>(w)];
        CHECK(differ == 1);
        CHECK((words[static_cast<size_t>(at) * ref::kLanes + p.lane] ^ other[static_cast<size_t>(at) * ref::kLanes + p.lane]) == p.xor_mask);
      }
    }
  }
  CHECK(temps_with_a_slot[0] >= 1 && temps_with_a_slot[1] >= 1);

  // the bounds of a plant and of the sweep count
  const Plant ok{0, 0, 2, 0, 1};
  CHECK(ref::plant_ok(ok) && ref::plant_ok(Plant{-1, 4, 7, 63, 0xffffffffu}));
  for (const Plant& bad : {Plant{-2, 0, 2, 0, 1}, Plant{0, -1, 2, 0, 1}, Plant{0, ref::kPhases, 2, 0, 1}, Plant{0, 0, -1, 0, 1},
                           Plant{0, 0, ref::kPlantSlots, 0, 1}, Plant{0, 0, 2, -1, 1}, Plant{0, 0, 2, ref::kLanes, 1}, Plant{0, 0, 2, 0, 0},
                           Plant{0, 0, 0, 0, 1}, Plant{0, 2, 4, 0, 1}, Plant{0, 4, 1, 0, 1}}) {
    CHECK(!ref::plant_ok(bad));
  }
  CHECK(!ref::sweeps_ok(0) && ref::sweeps_ok(1) && ref::sweeps_ok(1 << 16) && !ref::sweeps_ok((1 << 16) + 1) && !ref::sweeps_ok(-1));
  CHECK(ref::words_checked(4) == 4ull * 64 * (4 * 504 + 504));

  if (failures) return 1;
  std::puts("ok");
  return 0;
}
