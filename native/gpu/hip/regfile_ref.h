// The register-file check's host reference (bgc_diag_regfile): the pattern, the wave seed, the two march layouts, the
// rotate ring, the plant registers and the contents of a wave's 512 x 64 words after any phase, each written once.  No
// HIP dependency: regfile.hip's host code uses it to validate arguments and to answer bgc_diag_regfile_layout and
// bgc_diag_regfile_expected, tests/native/regfile_ref.cc exercises it alone, and the kernels' assembly, which cannot
// include it, states the same constants and is held to it by static_asserts and by the generated-data test.
//
// Registers are numbered 0..511: v0..v255 are 0..255 and a0..a255 are 256..511.  Words are [register][lane].
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace bgc_regfile {

constexpr int kRegs = 512, kLanes = 64, kWords = kRegs * kLanes;
constexpr int kTemps = 8;  // registers a layout keeps for the check's own use: expected value, scratch, counters, first bad

// Phases: 0..3 are the march's (layout = phase >> 1, pass = phase & 1), 4 is the rotate.
constexpr int kPhases = 5, kPhaseRotate = 4;

// What a march pass or the rotate fill writes: a hash of the wave seed and the lane, plus the register times an odd
// constant; pass 1 writes the inverse.  mix32 is a bijection and the constant is odd, so any two lanes of a register
// and any two registers of a lane differ, and across the two passes every bit of every cell holds both 0 and 1.
constexpr uint32_t kRegStep = 0x61c88647u, kWaveStep = 0x9e3779b9u, kMixA = 0x7feb352du, kMixB = 0x846ca68bu;

constexpr uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= kMixA;
  x ^= x >> 15;
  x *= kMixB;
  x ^= x >> 16;
  return x;
}
constexpr uint32_t wave_seed(uint32_t seed, uint32_t wave) { return mix32(seed + (wave + 1) * kWaveStep); }
constexpr uint32_t lane_hash(uint32_t wseed, uint32_t lane) { return mix32(wseed + lane); }
constexpr uint32_t pattern(uint32_t wseed, int reg, int lane, int pass) {
  return (lane_hash(wseed, static_cast<uint32_t>(lane)) + static_cast<uint32_t>(reg) * kRegStep) ^ (pass ? ~0u : 0u);
}

// Layout 0 keeps v0..v7 and marches the rest; layout 1 keeps v248..v255.  Together they march all 512.
constexpr int temp_base(int layout) { return layout == 0 ? 0 : 248; }
constexpr bool is_temp(int layout, int reg) { return reg >= temp_base(layout) && reg < temp_base(layout) + kTemps; }
constexpr int marched_regs(int /*layout*/) { return kRegs - kTemps; }

// The rotate ring: v8..v255, a0..a255 (v0..v7 are its temporaries, as in layout 0).  Ring index i is register
// kRingFirst + i.  A sweep moves the word at index i + 1 to index i, and the word at index 0 to the last.
constexpr int kRingFirst = 8, kRing = kRegs - kRingFirst;
constexpr int ring_reg(int index) { return kRingFirst + index; }
constexpr int ring_index(int reg) { return reg - kRingFirst; }
// where the word that the fill put into `reg` is after `sweeps` sweeps
constexpr int travelled_to(int reg, int sweeps) { return ring_reg(((ring_index(reg) - sweeps % kRing) + kRing) % kRing); }
// and which register's fill `reg` holds then
constexpr int came_from(int reg, int sweeps) { return ring_reg((ring_index(reg) + sweeps % kRing) % kRing); }

// A value plant names a slot of this list: the first and last VGPR and AGPR, one mid register of each half, and two
// registers of each layout's temporaries, which only the other layout can verify.
constexpr int kPlantSlots = 8;
constexpr int kPlantRegs[kPlantSlots] = {0, 5, 128, 250, 255, 256, 384, 511};
// whether `phase` holds a pattern in `reg` (a plant there is seen)
constexpr bool phase_holds(int phase, int reg) {
  return reg >= 0 && reg < kRegs && (phase == kPhaseRotate ? reg >= kRingFirst : phase >= 0 && phase < kPhaseRotate && !is_temp(phase >> 1, reg));
}

// A plant as the C ABI has it (bgc_regfile_plant); P needs wave, phase, slot, lane, xor_mask.
template <class P>
constexpr bool plant_ok(const P& p) {
  return p.wave >= -1 && p.phase >= 0 && p.phase < kPhases && p.slot >= 0 && p.slot < kPlantSlots && p.lane >= 0 && p.lane < kLanes &&
         p.xor_mask != 0 && phase_holds(p.phase, kPlantRegs[p.slot]);
}

constexpr bool sweeps_ok(int sweeps) { return sweeps >= 1 && sweeps <= (1 << 16); }

// words checked by a run of `waves` waves: four march passes of the marched registers, and the ring after the rotate
constexpr uint64_t words_checked(int waves) {
  return static_cast<uint64_t>(waves) * kLanes * (2 * (marched_regs(0) + marched_regs(1)) + kRing);
}

// What wave `wave` holds when phase `phase` is dumped: after the fill and the plants of a march phase, or after the
// rotate's fill, its plants and `sweeps` sweeps.  Registers the phase keeps for itself are 0.  words[reg * 64 + lane].
template <class P>
void expected(uint32_t seed, int wave, int phase, int sweeps, const P* plants, int n, uint32_t* words) {
  const uint32_t ws = wave_seed(seed, static_cast<uint32_t>(wave));
  const int pass = phase == kPhaseRotate ? 0 : phase & 1;
  for (int reg = 0; reg < kRegs; ++reg) {
    for (int lane = 0; lane < kLanes; ++lane) words[reg * kLanes + lane] = phase_holds(phase, reg) ? pattern(ws, reg, lane, pass) : 0u;
  }
  for (int j = 0; j < n; ++j) {
    const P& p = plants[j];
    if ((p.wave == -1 || p.wave == wave) && p.phase == phase) words[kPlantRegs[p.slot] * kLanes + p.lane] ^= p.xor_mask;
  }
  if (phase != kPhaseRotate) return;
  uint32_t* ring = words + kRingFirst * kLanes;
  const std::vector<uint32_t> filled(ring, ring + kRing * kLanes);
  for (int i = 0; i < kRing; ++i) {
    std::memcpy(ring + static_cast<size_t>(i) * kLanes, filled.data() + static_cast<size_t>(ring_index(came_from(ring_reg(i), sweeps))) * kLanes,
                kLanes * sizeof(uint32_t));
  }
}

}  // namespace bgc_regfile
