// pack_search.hpp — the host's arithmetic of md_pack_sketch_* and md_pack_choose_bases (mdeflate.h; capi_pack_search.cpp): the
// constants of the sketch, how an object is cut into segments, the pack order, the candidates of every target from the
// groups of equal (type, feature), and the choice among the scored pairs.  Plain C++: no device code, no md_ctx
// (tests/pack_search_check.cpp drives it alone under the sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mdeflate.h"
#include "pack_write.hpp"

namespace md {
namespace pks {

// ---- the sketch definition ----
constexpr uint32_t kFeatures = 4;
constexpr uint32_t kSeeds[kFeatures] = {0, 0x85EBCA6Bu, 0xC2B2AE35u, 0x27D4EB2Fu};
// an object is cut into segments of this many positions, one wavefront each (64 steps of 64 lanes)
constexpr uint32_t kSegPositions = 4096;
constexpr uint32_t kMaxWindow = 64;
constexpr uint64_t kMaxPairs = 0x7ffffff0ull;  // n * 4 * window at the most

// positions p with p + 16 <= len, and the segments they make
inline uint64_t positions(uint64_t len) { return len >= pkw::kBlock ? len - pkw::kBlock + 1 : 0; }
inline uint64_t segments(uint64_t len) { return (positions(len) + kSegPositions - 1) / kSegPositions; }
inline bool has_features(uint64_t len) { return len >= pkw::kBlock; }

// ---- md_pack_choose_bases ----
// Pack order: by (type, len descending, input index).  order[r] = the input index at rank r.  (type is 1 .. 4 and len at
// most MD_MAX_STREAM, below 2^32: one 64-bit key an object, so the sort moves no pointers.)
struct Keyed {
  uint64_t key;
  uint32_t at;
  bool operator<(const Keyed &o) const { return key != o.key ? key < o.key : at < o.at; }
};
inline void pack_order(size_t n, const md_pack_source *objs, uint64_t *order) {
  std::vector<Keyed> keys(n);
  for (size_t i = 0; i < n; i++) keys[i] = {(uint64_t)objs[i].type << 32 | (0xffffffffu - (uint32_t)objs[i].len), (uint32_t)i};
  std::sort(keys.begin(), keys.end());
  for (size_t r = 0; r < n; r++) order[r] = keys[r].at;
}

// The pairs that are scored, by ranks: pair k of target rank t, first[t] <= k < first[t + 1], is against the object at rank
// base[k]; a target's bases ascend.  A candidate of t for feature i is one of the at most `window` objects nearest in
// front of t in pack order with t's type and t's F_i; the union over the features counts each once.  An object shorter
// than 16 bytes has no features - whatever `features` holds for it - and a target shorter than 64 is not scored.
// features: kFeatures words an object, by INPUT index.
struct Pairs {
  std::vector<uint64_t> first;
  std::vector<uint32_t> base;
};
inline void candidates(size_t n, const md_pack_source *objs, const uint64_t *order, const uint32_t *features, uint32_t window, Pairs *out) {
  // per feature the ranks that have features, grouped by (type, F_i) and ascending within a group; where[i][r]: rank r's place
  std::vector<Keyed> group[kFeatures];
  std::vector<uint32_t> where[kFeatures];
  for (uint32_t i = 0; i < kFeatures; i++) {
    group[i].reserve(n);
    for (size_t r = 0; r < n; r++) {
      const md_pack_source &o = objs[order[r]];
      if (has_features(o.len)) group[i].push_back({(uint64_t)o.type << 32 | features[kFeatures * order[r] + i], (uint32_t)r});
    }
    std::sort(group[i].begin(), group[i].end());
    where[i].assign(n, 0);
    for (size_t k = 0; k < group[i].size(); k++) where[i][group[i][k].at] = (uint32_t)k;
  }
  out->first.assign(n + 1, 0);
  out->base.clear();
  std::vector<uint32_t> found;
  for (size_t t = 0; t < n; t++) {
    out->first[t] = out->base.size();
    static_assert(pkw::kDeltaMinTarget >= pkw::kBlock, "a target has features");
    if (objs[order[t]].len < pkw::kDeltaMinTarget) continue;
    found.clear();
    for (uint32_t i = 0; i < kFeatures; i++) {
      const size_t k = where[i][t];
      for (size_t back = 1; back <= window && back <= k && group[i][k - back].key == group[i][k].key; back++) found.push_back(group[i][k - back].at);
    }
    std::sort(found.begin(), found.end());
    out->base.insert(out->base.end(), found.begin(), std::unique(found.begin(), found.end()));
  }
  out->first[n] = out->base.size();
}

// The choice, in pack order: among a target's pairs whose delta fitted (fitted[k] != 0, its length len[k]) and whose base's
// depth is below max_depth (0: no limit) the smallest delta, the earlier base on a tie; depth = the base's + 1.  No such
// pair: the object is whole, depth 0.  base[r] = the chosen base's rank or MD_PACK_NO_BASE.  Returns the bases chosen.
inline uint64_t choose(size_t n, const Pairs &pairs, const uint64_t *len, const uint8_t *fitted, uint32_t max_depth, uint64_t *base,
                       uint32_t *depth) {
  uint64_t chosen = 0;
  for (size_t t = 0; t < n; t++) {
    base[t] = MD_PACK_NO_BASE, depth[t] = 0;
    uint64_t best = UINT64_MAX;
    for (uint64_t k = pairs.first[t]; k < pairs.first[t + 1]; k++) {
      const uint32_t b = pairs.base[k];  // (b < t: a candidate stands in front of its target)
      if (!fitted[k] || (max_depth && depth[b] >= max_depth) || len[k] >= best) continue;
      best = len[k], base[t] = b, depth[t] = depth[b] + 1;
    }
    chosen += base[t] != MD_PACK_NO_BASE;
  }
  return chosen;
}

}  // namespace pks
}  // namespace md
