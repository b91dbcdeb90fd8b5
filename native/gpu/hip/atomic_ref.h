// The atomic check's operands, its mapping of (wave, round, lane) to table elements, and the host referee
// (gpu_diag.h, "Atomics").  No HIP dependency: atomic.hip includes it for both sides, and a plain C++17 program
// can include it alone to run the referee, under a sanitizer for instance.
//
//  * The operands, the initial values, the rows and the word indices are written once, as functions that the
//    kernels and the host both call.
//  * expected() replays every operation of a launch in the order of the pairs, in integer arithmetic or in float
//    additions whose every partial sum is an integer the format holds exactly, so the order does not matter.  Of
//    what the order does decide (who wins a cas, which ticket a puller draws) it gives one admissible outcome, and
//    judge() checks those by their property instead: one winner per element whose id the element holds, a counter
//    equal to its pullers and an order array that is a permutation of their ids.
//  * Hazards on the host: every sum that may wrap is unsigned, a float becomes an integer only after a range check,
//    and every index is below the size that make_layout() computed for it.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "gpu_diag.h"

#if defined(__HIPCC__)
#define BGC_ATOMIC_HD __host__ __device__ __forceinline__
#else
#define BGC_ATOMIC_HD inline
#endif

namespace bgc_atomic {

using Layout = bgc_atomic_layout;

constexpr int kClasses = BGC_ATOMIC_CLASSES;
constexpr int kRateClasses = BGC_ATOMIC_RATE_CLASSES;
constexpr uint32_t kEmpty = BGC_ATOMIC_EMPTY;
constexpr int kRateRows = 64;       // rows of a rate group
constexpr int kRateAdders = 8;      // waves of a rate group
constexpr uint32_t kRateStep = 0x9e3779b9U;
enum IntWord { kAdd, kSmin, kUmax, kAnd, kOr, kXor };
enum LdsWord { kLdsAdd, kLdsTicket, kLdsMax, kLdsMin, kLdsAnd, kLdsOr, kLdsXor, kLdsAddF32, kLdsCas, kLdsWords };
enum Order { kOrderOwn, kOrderShared, kOrderLds };

// 32-bit words of a class's element, the words a plant can name, and the cap on the operations of a SHARED element
BGC_ATOMIC_HD constexpr int class_words(int cls) {
  constexpr int words[kClasses] = {6, 2, 1, 2, 2, 1, 1, kLdsWords};
  return words[cls];
}
BGC_ATOMIC_HD constexpr int class_ops(int cls) {
  constexpr int ops[kClasses] = {6, 1, 1, 1, 2, 1, 1, kLdsWords};
  return ops[cls];
}
BGC_ATOMIC_HD constexpr uint32_t class_cap(int cls) {
  constexpr uint32_t cap[kClasses] = {4096, 4096, 4096, 4096, 128, 64, 64, 0};
  return cap[cls];
}
BGC_ATOMIC_HD constexpr bool is_64bit(int cls) { return cls == BGC_ATOMIC_INT64 || cls == BGC_ATOMIC_F64; }

BGC_ATOMIC_HD uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// operand word k of (class, wave, round, lane); the inner hash depends on (seed, class, k) alone, and a loop over waves,
// rounds and lanes may compute it once
BGC_ATOMIC_HD uint32_t class_key(uint32_t seed, int cls, int k) { return mix32(seed ^ mix32(static_cast<uint32_t>(cls << 4 | k))); }
BGC_ATOMIC_HD uint32_t operand_of(uint32_t key, uint32_t wave, int round, int lane) {
  return mix32(key ^ (wave << 12 | static_cast<uint32_t>(round) << 6 | static_cast<uint32_t>(lane)));
}
BGC_ATOMIC_HD uint32_t operand(uint32_t seed, int cls, int k, uint32_t wave, int round, int lane) {
  return operand_of(class_key(seed, cls, k), wave, round, lane);
}
BGC_ATOMIC_HD int f32_value(uint32_t h) { return static_cast<int>(h % 4095) - 2047; }
BGC_ATOMIC_HD int64_t f64_value(uint32_t h) { return static_cast<int64_t>(h >> 6) - (1 << 25); }
BGC_ATOMIC_HD int trit(uint32_t h) { return static_cast<int>(h % 3) - 1; }
BGC_ATOMIC_HD uint32_t bf16_of_trit(int t) { return t > 0 ? 0x3f80u : t < 0 ? 0xbf80u : 0u; }
BGC_ATOMIC_HD uint32_t f16_of_trit(int t) { return t > 0 ? 0x3c00u : t < 0 ? 0xbc00u : 0u; }
BGC_ATOMIC_HD uint32_t pk_bf16_trits(int lo, int hi) { return bf16_of_trit(lo) | bf16_of_trit(hi) << 16; }
BGC_ATOMIC_HD uint32_t pk_f16_trits(int lo, int hi) { return f16_of_trit(lo) | f16_of_trit(hi) << 16; }

// what a word of the int32 class (and the LDS word that does the same) starts from
BGC_ATOMIC_HD uint32_t int_init(int word) { return word == kSmin ? 0x7fffffffU : word == kAnd ? 0xffffffffU : 0u; }
BGC_ATOMIC_HD uint32_t lds_init(int word) {
  return word == kLdsMin ? 0x7fffffffU : word == kLdsAnd ? 0xffffffffU : word == kLdsCas ? kEmpty : 0u;
}

// the row of a class's table that pair (wave, round) works on
BGC_ATOMIC_HD uint32_t row_of(const Layout& L, int placement, int cls, uint32_t wave, int round) {
  if (placement == BGC_ATOMIC_OWN) return 2 * (wave / 4) + ((wave + static_cast<uint32_t>(round)) & 1);
  return (wave * static_cast<uint32_t>(L.rounds) + static_cast<uint32_t>(round)) % L.rows[placement][cls];
}
// word k of element (row, lane) of a 32-bit class, the element of a 64-bit class: words from the start of the placement's table
BGC_ATOMIC_HD uint64_t word_at(const Layout& L, int placement, int cls, int k, uint32_t row, int lane) {
  if (is_64bit(cls)) return L.table_off[placement][cls] + (static_cast<uint64_t>(row) * 64 + static_cast<uint64_t>(lane)) * 2 + static_cast<uint64_t>(k);
  return L.table_off[placement][cls] + (static_cast<uint64_t>(k) * L.rows[placement][cls] + row) * 64 + static_cast<uint64_t>(lane);
}
// slot 0 of the order array of element (row, lane)
BGC_ATOMIC_HD uint64_t order_at(const Layout& L, int order, uint32_t row, int lane) {
  return (static_cast<uint64_t>(row) * 64 + static_cast<uint64_t>(lane)) * L.order_cap[order];
}

// the rate phase: the operand hash of (class, wave, lane), the visits of row `row` in `iters` iterations, the wave of adder a of group g
BGC_ATOMIC_HD uint32_t rate_operand(uint32_t seed, int cls, uint32_t wave, int lane) {
  return mix32(mix32(seed ^ mix32(0x100u | static_cast<uint32_t>(cls))) ^ (wave << 6 | static_cast<uint32_t>(lane)));
}
BGC_ATOMIC_HD uint32_t rate_visits(int row, int iters) { return row < iters ? static_cast<uint32_t>(iters - row + kRateRows - 1) / kRateRows : 0u; }
BGC_ATOMIC_HD uint32_t rate_group(uint32_t wave) { return (wave / 4 / kRateAdders) * 4 + wave % 4; }
BGC_ATOMIC_HD uint32_t rate_wave(uint32_t group, int adder) { return ((group / 4) * kRateAdders + static_cast<uint32_t>(adder)) * 4 + group % 4; }

// ---------------------------------------------------------------------------------------------
// host

inline bool layout_args_ok(int grid, int rate_grid, int rounds) {
  return grid >= 1 && grid <= 16384 && rate_grid >= 8 && rate_grid <= 4096 && rate_grid % 8 == 0 && rounds >= 1 && rounds <= 64;
}

inline void make_layout(int grid, int rate_grid, int rounds, Layout* L) {
  memset(L, 0, sizeof(*L));
  L->grid = grid;
  L->rate_grid = rate_grid;
  L->rounds = rounds;
  L->waves = 4 * grid;
  L->pairs = static_cast<uint32_t>(L->waves) * static_cast<uint32_t>(rounds);
  uint64_t table_words[2] = {0, 0};
  for (int pl = 0; pl < 2; ++pl) {
    for (int c = 0; c < kClasses; ++c) {
      const uint32_t rows = pl == BGC_ATOMIC_OWN ? 2u * static_cast<uint32_t>(grid) : c == BGC_ATOMIC_LDS ? 0u : (L->pairs + class_cap(c) - 1) / class_cap(c);
      L->rows[pl][c] = rows;
      L->table_off[pl][c] = table_words[pl];
      table_words[pl] += static_cast<uint64_t>(rows) * 64 * static_cast<uint64_t>(class_words(c));
    }
  }
  const uint32_t shared_rows = L->rows[BGC_ATOMIC_SHARED][BGC_ATOMIC_TICKET];
  L->order_cap[kOrderOwn] = L->order_cap[kOrderLds] = 2u * static_cast<uint32_t>(rounds);
  L->order_cap[kOrderShared] = (L->pairs + shared_rows - 1) / shared_rows;
  const uint64_t own_order = static_cast<uint64_t>(2 * grid) * 64 * L->order_cap[kOrderOwn];
  const uint64_t words[BGC_ATOMIC_DATA_SECTIONS] = {table_words[0],
                                                    table_words[1],
                                                    3ULL * L->pairs * 2,
                                                    own_order,
                                                    static_cast<uint64_t>(shared_rows) * 64 * L->order_cap[kOrderShared],
                                                    own_order,
                                                    static_cast<uint64_t>(grid),
                                                    static_cast<uint64_t>(kRateClasses) * static_cast<uint64_t>(rate_grid)};
  for (int s = 0; s < BGC_ATOMIC_DATA_SECTIONS; ++s) {
    L->data_off[s] = L->total_words;
    L->data_words[s] = words[s];
    L->total_words += words[s] + (words[s] & 1);  // every section starts at a multiple of 8 bytes
  }
}

inline void init_table(const Layout& L, int placement, uint32_t* table) {
  for (int c = 0; c < kClasses; ++c) {
    const uint64_t per_word = static_cast<uint64_t>(L.rows[placement][c]) * 64;
    for (int k = 0; k < class_words(c); ++k) {
      const uint32_t v = c == BGC_ATOMIC_INT32 ? int_init(k) : c == BGC_ATOMIC_LDS ? lds_init(k) : c == BGC_ATOMIC_CAS ? kEmpty : 0u;
      // a 64-bit class starts from 0 in both words, so its interleaved layout needs no case of its own
      std::fill_n(table + L.table_off[placement][c] + static_cast<uint64_t>(k) * per_word, per_word, v);
    }
  }
}

inline float f32_of(uint32_t bits) { return __builtin_bit_cast(float, bits); }
inline uint32_t bits_of(float x) { return __builtin_bit_cast(uint32_t, x); }
inline double f64_of(uint64_t bits) { return __builtin_bit_cast(double, bits); }
inline uint64_t bits_of(double x) { return __builtin_bit_cast(uint64_t, x); }

// A half of a packed word as the number it encodes, and an integer of magnitude <= 256 (bf16) or 2048 (fp16) as a half.
inline double bf16_value(uint32_t h) { return static_cast<double>(f32_of((h & 0xffffU) << 16)); }
inline double f16_value(uint32_t h) {
  h &= 0xffffU;
  const int e = static_cast<int>((h >> 10) & 31);
  const double m = static_cast<double>(h & 0x3ff);
  const double mag = e == 0 ? ldexp(m, -24) : e == 31 ? (m == 0 ? static_cast<double>(INFINITY) : static_cast<double>(NAN)) : ldexp(1024.0 + m, e - 25);
  return (h & 0x8000) ? -mag : mag;
}
inline uint32_t bf16_of_int(int v) { return bits_of(static_cast<float>(v)) >> 16; }
inline uint32_t f16_of_int(int v) {
  if (v == 0) return 0;
  const uint32_t b = bits_of(static_cast<float>(v));
  return (b >> 16 & 0x8000U) | (((b >> 23 & 0xff) - 112) << 10) | (b >> 13 & 0x3ff);
}
// a float that holds an integer, as that integer; 0 for anything else
inline int64_t integer_of(double x) { return x == x && fabs(x) < 9.0e18 ? static_cast<int64_t>(x) : 0; }

struct Tap {
  int times = 1;
  uint32_t mask = 0;
};

// the plants of a list by the atomic they name; of several on one atomic the first applies
class Plants {
 public:
  Plants(const bgc_atomic_plant* p, int n) {
    for (int i = 0; i < n; ++i) by_key_.emplace(key(p[i].placement, p[i].cls, p[i].op, static_cast<uint32_t>(p[i].wave), p[i].round, p[i].lane), Tap{p[i].times, p[i].xor_mask});
  }
  Tap at(int placement, int cls, int op, uint32_t wave, int round, int lane) const {
    if (by_key_.empty()) return Tap{};
    const auto it = by_key_.find(key(placement, cls, op, wave, round, lane));
    return it == by_key_.end() ? Tap{} : it->second;
  }

 private:
  static uint64_t key(int placement, int cls, int op, uint32_t wave, int round, int lane) {
    return static_cast<uint64_t>(placement) << 60 | static_cast<uint64_t>(cls) << 56 | static_cast<uint64_t>(op) << 48 | static_cast<uint64_t>(wave) << 16 |
           static_cast<uint64_t>(round) << 8 | static_cast<uint64_t>(lane);
  }
  std::map<uint64_t, Tap> by_key_;
};

// The sections of a data block of L.total_words words.
struct Data {
  uint32_t* table[2];
  uint64_t* ballots[3];  // OWN, SHARED, LDS: one per pair
  uint32_t* order[3];
  int32_t* cu_keys;
  int32_t* rate_cu_keys;
  Data(const Layout& L, uint32_t* words) {
    table[0] = words + L.data_off[BGC_ATOMIC_DATA_OWN];
    table[1] = words + L.data_off[BGC_ATOMIC_DATA_SHARED];
    for (int k = 0; k < 3; ++k) {
      ballots[k] = reinterpret_cast<uint64_t*>(words + L.data_off[BGC_ATOMIC_DATA_BALLOTS]) + static_cast<uint64_t>(k) * L.pairs;
      order[k] = words + L.data_off[BGC_ATOMIC_DATA_ORDER_OWN + k];
    }
    cu_keys = reinterpret_cast<int32_t*>(words + L.data_off[BGC_ATOMIC_DATA_CU_KEYS]);
    rate_cu_keys = reinterpret_cast<int32_t*>(words + L.data_off[BGC_ATOMIC_DATA_RATE_CU_KEYS]);
  }
};

// The referee's tables, ballots and order arrays for a launch, `plants` applied; `words` holds L.total_words.
// Returns the tickets that fell out of range (a doubled pull draws one).
inline uint64_t expected(const Layout& L, uint32_t seed, const bgc_atomic_plant* plants, int n, uint32_t* words) {
  std::fill_n(words, L.total_words, 0u);
  Data d(L, words);
  init_table(L, BGC_ATOMIC_OWN, d.table[0]);
  init_table(L, BGC_ATOMIC_SHARED, d.table[1]);
  std::fill_n(d.cu_keys, L.data_words[BGC_ATOMIC_DATA_CU_KEYS], -1);
  std::fill_n(d.rate_cu_keys, L.data_words[BGC_ATOMIC_DATA_RATE_CU_KEYS], -1);
  const Plants taps(plants, n);
  uint64_t out_of_range = 0;
  uint32_t key[kClasses][kLdsWords] = {};
  for (int c = 0; c < kClasses; ++c) {
    for (int k = 0; k < class_ops(c) || k < class_words(c); ++k) key[c][k] = class_key(seed, c, k);
  }
  for (uint32_t w = 0; w < static_cast<uint32_t>(L.waves); ++w) {
    for (int r = 0; r < L.rounds; ++r) {
      const uint32_t pair = w * static_cast<uint32_t>(L.rounds) + static_cast<uint32_t>(r);
      for (int pl = 0; pl < 2; ++pl) {
        uint32_t* t = d.table[pl];
        uint32_t at_row[kClasses] = {};
        for (int c = 0; c < kClasses; ++c) at_row[c] = L.rows[pl][c] ? row_of(L, pl, c, w, r) : 0;
        for (int lane = 0; lane < 64; ++lane) {
          const uint32_t id = pair * 64 + static_cast<uint32_t>(lane);
          // `times` times f(operand word with the mask in it)
          auto issue = [&](int cls, int op, uint32_t raw, auto&& f) {
            const Tap tap = taps.at(pl, cls, op, w, r, lane);
            for (int i = 0; i < tap.times; ++i) f(raw ^ tap.mask);
          };
          auto int_word = [&](int cls, int k, int kind) {
            uint32_t& x = t[word_at(L, pl, cls, k, at_row[cls], lane)];
            issue(cls, k, operand_of(key[cls][k], w, r, lane), [&](uint32_t a) {
              switch (kind) {
                case kAdd: x += a; break;
                case kSmin: x = static_cast<int32_t>(a) < static_cast<int32_t>(x) ? a : x; break;
                case kUmax: x = a > x ? a : x; break;
                case kAnd: x &= a; break;
                case kOr: x |= a; break;
                default: x ^= a; break;
              }
            });
          };
          auto f32_word = [&](int cls, int k) {
            uint32_t& x = t[word_at(L, pl, cls, k, at_row[cls], lane)];
            issue(cls, k, operand_of(key[cls][k], w, r, lane), [&](uint32_t a) { x = bits_of(f32_of(x) + static_cast<float>(f32_value(a))); });
          };
          auto ticket = [&](int cls, int k, int order) {
            const uint32_t row = at_row[cls];
            uint32_t& counter = t[word_at(L, pl, cls, k, row, lane)];
            issue(cls, k, id, [&](uint32_t a) {
              const uint32_t drawn = counter++;
              if (drawn < L.order_cap[order]) {
                d.order[order][order_at(L, order, row, lane) + drawn] = a + 1;
              } else {
                out_of_range++;
              }
            });
          };
          auto cas = [&](int cls, int k, int which) {
            uint32_t& x = t[word_at(L, pl, cls, k, at_row[cls], lane)];
            issue(cls, k, id, [&](uint32_t a) {
              if (x == kEmpty) {
                x = a;
                d.ballots[which][pair] |= 1ULL << lane;
              }
            });
          };
          for (int k = 0; k < 6; ++k) int_word(BGC_ATOMIC_INT32, k, k);
          {
            const uint64_t at = word_at(L, pl, BGC_ATOMIC_INT64, 0, at_row[BGC_ATOMIC_INT64], lane);
            const uint64_t hi = static_cast<uint64_t>(operand_of(key[BGC_ATOMIC_INT64][1], w, r, lane)) << 32;
            issue(BGC_ATOMIC_INT64, 0, operand_of(key[BGC_ATOMIC_INT64][0], w, r, lane), [&](uint32_t lo) {
              const uint64_t sum = (static_cast<uint64_t>(t[at + 1]) << 32 | t[at]) + (hi | lo);
              t[at] = static_cast<uint32_t>(sum);
              t[at + 1] = static_cast<uint32_t>(sum >> 32);
            });
          }
          f32_word(BGC_ATOMIC_F32, 0);
          {
            const uint64_t at = word_at(L, pl, BGC_ATOMIC_F64, 0, at_row[BGC_ATOMIC_F64], lane);
            issue(BGC_ATOMIC_F64, 0, operand_of(key[BGC_ATOMIC_F64][0], w, r, lane), [&](uint32_t a) {
              const uint64_t sum = bits_of(f64_of(static_cast<uint64_t>(t[at + 1]) << 32 | t[at]) + static_cast<double>(f64_value(a)));
              t[at] = static_cast<uint32_t>(sum);
              t[at + 1] = static_cast<uint32_t>(sum >> 32);
            });
          }
          for (int k = 0; k < 2; ++k) {
            uint32_t& x = t[word_at(L, pl, BGC_ATOMIC_PK16, k, at_row[BGC_ATOMIC_PK16], lane)];
            issue(BGC_ATOMIC_PK16, k, operand_of(key[BGC_ATOMIC_PK16][k], w, r, lane), [&](uint32_t a) {
              const double lo = (k == 0 ? bf16_value(x) : f16_value(x)) + trit(a), hi = (k == 0 ? bf16_value(x >> 16) : f16_value(x >> 16)) + trit(a >> 16);
              const int l = static_cast<int>(integer_of(lo)), h = static_cast<int>(integer_of(hi));
              x = k == 0 ? (bf16_of_int(l) | bf16_of_int(h) << 16) : (f16_of_int(l) | f16_of_int(h) << 16);
            });
          }
          cas(BGC_ATOMIC_CAS, 0, pl);
          ticket(BGC_ATOMIC_TICKET, 0, pl == BGC_ATOMIC_OWN ? kOrderOwn : kOrderShared);
          if (pl == BGC_ATOMIC_OWN) {
            int_word(BGC_ATOMIC_LDS, kLdsAdd, kAdd);
            ticket(BGC_ATOMIC_LDS, kLdsTicket, kOrderLds);
            int_word(BGC_ATOMIC_LDS, kLdsMax, kUmax);
            int_word(BGC_ATOMIC_LDS, kLdsMin, kSmin);
            int_word(BGC_ATOMIC_LDS, kLdsAnd, kAnd);
            int_word(BGC_ATOMIC_LDS, kLdsOr, kOr);
            int_word(BGC_ATOMIC_LDS, kLdsXor, kXor);
            f32_word(BGC_ATOMIC_LDS, kLdsAddF32);
            cas(BGC_ATOMIC_LDS, kLdsCas, 2);
          }
        }
      }
    }
  }
  return out_of_range;
}

// what a word is, for the way it is judged and for first_bad_delta
enum Kind { kBits, kAddU32, kAddU64, kAddF32, kAddF64, kAddBf16, kAddF16, kCas, kTicket };
inline Kind kind_of(int cls, int k) {
  switch (cls) {
    case BGC_ATOMIC_INT32: return k == kAdd ? kAddU32 : kBits;
    case BGC_ATOMIC_INT64: return kAddU64;
    case BGC_ATOMIC_F32: return kAddF32;
    case BGC_ATOMIC_F64: return kAddF64;
    case BGC_ATOMIC_PK16: return k == 0 ? kAddBf16 : kAddF16;
    case BGC_ATOMIC_CAS: return kCas;
    case BGC_ATOMIC_TICKET: return kTicket;
    default: return k == kLdsAdd ? kAddU32 : k == kLdsTicket ? kTicket : k == kLdsAddF32 ? kAddF32 : k == kLdsCas ? kCas : kBits;
  }
}

// The verdict on the data of a run (`found`, L.total_words words; its CU keys are read, its rate CU keys are not):
// mismatches, first_bad_*, bad_cus, bad_cu_keys, cus_seen and values_checked of `out`, which the caller has zeroed
// (first_bad_placement, _class, _op and _element -1).
inline void judge(const Layout& L, uint32_t seed, const uint32_t* found, bgc_atomic_result* out) {
  std::vector<uint32_t> want_words(L.total_words);
  expected(L, seed, nullptr, 0, want_words.data());
  const Data want(L, want_words.data()), got(L, const_cast<uint32_t*>(found));
  std::vector<char> bad_wg(static_cast<size_t>(L.grid), 0);
  auto note = [&](int pl, int cls, int k, uint32_t row, int lane, uint64_t x, int64_t delta) {
    out->mismatches[pl][cls]++;
    if (pl == BGC_ATOMIC_OWN) bad_wg[row / 2] = 1;
    if (out->first_bad_placement >= 0) return;
    out->first_bad_placement = pl;
    out->first_bad_class = cls;
    out->first_bad_op = k;
    out->first_bad_element = static_cast<int64_t>(row) * 64 + lane;
    out->first_bad_xor = x;
    out->first_bad_delta = delta;
  };
  // the winners of every cas element and the pair that won it last, from the ballots
  auto winners_of = [&](int pl, int cls, const uint64_t* ballots, std::vector<uint32_t>* count, std::vector<uint32_t>* id) {
    const size_t elements = static_cast<size_t>(L.rows[pl][cls]) * 64;
    count->assign(elements, 0);
    id->assign(elements, kEmpty);
    for (uint32_t w = 0; w < static_cast<uint32_t>(L.waves); ++w) {
      for (int r = 0; r < L.rounds; ++r) {
        const uint32_t pair = w * static_cast<uint32_t>(L.rounds) + static_cast<uint32_t>(r), row = row_of(L, pl, cls, w, r);
        for (int lane = 0; ballots[pair] && lane < 64; ++lane) {
          if (!(ballots[pair] >> lane & 1)) continue;
          (*count)[static_cast<size_t>(row) * 64 + lane]++;
          (*id)[static_cast<size_t>(row) * 64 + lane] = pair * 64 + static_cast<uint32_t>(lane);
        }
      }
    }
  };
  std::vector<uint32_t> count, id, slots;
  for (int pl = 0; pl < 2; ++pl) {
    for (int c = 0; c < kClasses; ++c) {
      const uint32_t rows = L.rows[pl][c];
      if (rows == 0) continue;
      const int values = is_64bit(c) ? 1 : class_words(c);
      for (int k = 0; k < values; ++k) {
        const Kind kind = kind_of(c, k);
        const int order = c == BGC_ATOMIC_LDS ? kOrderLds : pl == BGC_ATOMIC_OWN ? kOrderOwn : kOrderShared;
        if (kind == kCas) winners_of(pl, c, got.ballots[c == BGC_ATOMIC_LDS ? 2 : pl], &count, &id);
        for (uint32_t row = 0; row < rows; ++row) {
          for (int lane = 0; lane < 64; ++lane) {
            const uint64_t at = word_at(L, pl, c, k, row, lane);
            const uint32_t g = got.table[pl][at], e = want.table[pl][at];
            switch (kind) {
              case kCas: {
                const size_t el = static_cast<size_t>(row) * 64 + lane;
                if (count[el] != 1 || g != id[el]) note(pl, c, k, row, lane, 0, 0);
                break;
              }
              case kTicket: {
                const uint32_t cap = L.order_cap[order];
                const uint64_t first = order_at(L, order, row, lane);
                bool ok = g == e && e <= cap;
                if (ok) {  // the slots in ascending order: the empty ones, then the pullers' id + 1 as the referee wrote them
                  slots.assign(got.order[order] + first, got.order[order] + first + cap);
                  std::sort(slots.begin(), slots.end());
                  for (uint32_t s = 0; ok && s < cap; ++s) ok = slots[s] == (s < cap - e ? 0u : want.order[order][first + s - (cap - e)]);
                }
                if (!ok) note(pl, c, k, row, lane, 0, 0);
                break;
              }
              case kAddU64:
              case kAddF64: {
                const uint64_t g64 = static_cast<uint64_t>(got.table[pl][at + 1]) << 32 | g, e64 = static_cast<uint64_t>(want.table[pl][at + 1]) << 32 | e;
                if (g64 == e64) break;
                const int64_t delta = kind == kAddU64 ? static_cast<int64_t>(g64 - e64) : integer_of(f64_of(g64)) - integer_of(f64_of(e64));
                note(pl, c, k, row, lane, g64 ^ e64, delta);
                break;
              }
              default: {
                if (g == e) break;
                int64_t delta = 0;
                if (kind == kAddU32) delta = static_cast<int32_t>(g - e);
                if (kind == kAddF32) delta = integer_of(f32_of(g)) - integer_of(f32_of(e));
                if (kind == kAddBf16 || kind == kAddF16) {
                  auto value = [&](uint32_t half) { return integer_of(kind == kAddBf16 ? bf16_value(half) : f16_value(half)); };
                  delta = (g & 0xffff) != (e & 0xffff) ? value(g) - value(e) : value(g >> 16) - value(e >> 16);
                }
                note(pl, c, k, row, lane, g ^ e, delta);
              }
            }
          }
        }
      }
    }
  }
  std::vector<int> keys(got.cu_keys, got.cu_keys + L.grid), bad_keys;
  for (int b = 0; b < L.grid; ++b) {
    if (bad_wg[static_cast<size_t>(b)]) bad_keys.push_back(keys[static_cast<size_t>(b)]);
  }
  std::sort(keys.begin(), keys.end());
  out->cus_seen = static_cast<int>(std::unique(keys.begin(), keys.end()) - keys.begin());
  std::sort(bad_keys.begin(), bad_keys.end());
  bad_keys.erase(std::unique(bad_keys.begin(), bad_keys.end()), bad_keys.end());
  for (int key : bad_keys) {
    if (out->bad_cus < 64) out->bad_cu_keys[out->bad_cus] = key;
    out->bad_cus++;
  }
  out->values_checked = L.data_words[BGC_ATOMIC_DATA_OWN] + L.data_words[BGC_ATOMIC_DATA_SHARED] + L.data_words[BGC_ATOMIC_DATA_ORDER_OWN] +
                        L.data_words[BGC_ATOMIC_DATA_ORDER_SHARED] + L.data_words[BGC_ATOMIC_DATA_ORDER_LDS];
}

// ---------------------------------------------------------------------------------------------
// the rate phase's closed forms

inline uint64_t rate_words(int rate_grid, int cls) {
  const uint64_t groups = static_cast<uint64_t>(rate_grid) / kRateAdders * 4;
  return cls == BGC_ATOMIC_RATE_RTN ? groups : groups * kRateRows * 64;
}

// The end values of class `cls` after `iters` iterations: rate_words() words.
inline void rate_expected(uint32_t seed, int rate_grid, int iters, int cls, uint32_t* out) {
  const uint32_t groups = static_cast<uint32_t>(rate_grid) / kRateAdders * 4;
  for (uint32_t g = 0; g < groups; ++g) {
    if (cls == BGC_ATOMIC_RATE_RTN) {
      out[g] = static_cast<uint32_t>(kRateAdders) * static_cast<uint32_t>(iters);
      continue;
    }
    for (int lane = 0; lane < 64; ++lane) {
      uint32_t sum_h = 0;
      int sum_lo = 0, sum_hi = 0;
      for (int a = 0; a < kRateAdders; ++a) {
        const uint32_t h = rate_operand(seed, cls, rate_wave(g, a), lane);
        sum_h += h;
        sum_lo += trit(h);
        sum_hi += trit(h >> 16);
      }
      for (int row = 0; row < kRateRows; ++row) {
        const uint32_t visits = rate_visits(row, iters);
        // the iterations that visit the row are row + 64 j: their sum, modulo 2^32
        const uint32_t sum_i = visits * static_cast<uint32_t>(row) + kRateRows * static_cast<uint32_t>(static_cast<uint64_t>(visits) * (visits ? visits - 1 : 0) / 2);
        const int lo = (visits & 1) ? sum_lo : 0, hi = (visits & 1) ? sum_hi : 0;
        out[(static_cast<size_t>(g) * kRateRows + static_cast<size_t>(row)) * 64 + static_cast<size_t>(lane)] =
            cls == BGC_ATOMIC_RATE_F32       ? bits_of(static_cast<float>(lo))
            : cls == BGC_ATOMIC_RATE_PK_BF16 ? (bf16_of_int(lo) | bf16_of_int(hi) << 16)
                                             : visits * sum_h + static_cast<uint32_t>(kRateAdders) * kRateStep * sum_i;
      }
    }
  }
}

}  // namespace bgc_atomic
