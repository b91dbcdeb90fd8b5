// The resourceVersion splice of kube-lite's commit path: an event line is serialized
// before the commit-order lock around a placeholder, and the digits assigned under the
// lock replace it in the same buffer (server.cc: prepare_commit, commit_locked,
// erase_locked).
#pragma once

#include <string>
#include <string_view>

namespace bgc::apiserver {

// Replaces line[at, at + len) by `digits` in place.  The text behind it moves once; the
// buffer is reallocated only when the digits are longer than what they replace and the
// capacity has no room for the difference (callers reserve kRvSpliceSlack beyond the dump).
inline void splice_rv(std::string& line, size_t at, size_t len, std::string_view digits) {
  line.replace(at, len, digits.data(), digits.size());
}

// Longest resourceVersion (20 decimal digits of a uint64, or "kl." + 13 base-36 digits).
constexpr size_t kRvSpliceSlack = 20;

}  // namespace bgc::apiserver
