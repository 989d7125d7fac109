// pack_diff.hpp — how two trees of a git pack are diffed (md_pack_diff; the rules are mdeflate.h's, read off git's canon_mode,
// base_name_compare and the merge of diff_tree).  The rules live here once: the kernels (pack_diff_kernels.hip) and the host
// check of the tests (tests/pack_diff_check.cpp) run these very functions.  Plain C++ with no HIP in it, as pack_graph.hpp,
// whose parse rules it stands on.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pack_graph.hpp"

#define MD_PD_FN MD_PG_FN

namespace md {
namespace pd {

constexpr uint32_t kNone = 0xffffffffu;            // MD_TREE_NONE: the empty tree as a side of a pair, no parent record
constexpr uint32_t kFlagTree = 1, kFlagOpaque = 2;  // MD_TREE_CHANGE_TREE, MD_TREE_CHANGE_OPAQUE
constexpr uint32_t kDirMode = 0040000;

// git's canon_mode of an entry's mode
MD_PD_FN uint32_t canon_mode(uint32_t m) {
  const uint32_t fmt = m & 0170000;
  if (fmt == 0100000) return (m & 0100) ? 0100755u : 0100644u;
  if (fmt == 0120000) return 0120000u;
  if (fmt == 0040000) return 0040000u;
  return 0160000u;
}
MD_PD_FN bool is_dir(uint32_t canon) { return canon == kDirMode; }

// One entry of a tree where it lies: it starts at `start`, its name is tree[name, nul), its 20 bytes follow the NUL; mode is
// canonical.  The table kernel writes one a row.
struct Entry {
  uint32_t start, name, nul, mode;
};

// The canonical mode of the entry that starts at a[s] and whose name ends with the NUL at a[nul], parsed as
// pack_graph.hpp's tree_entry_kind parses it (32 bits, wrapping); 0: malformed (no canonical mode is 0)
MD_PD_FN uint32_t entry_mode(const uint8_t *a, uint64_t s, uint64_t nul) {
  if (pg::tree_entry_kind(a, s, nul) == pg::kMalformed) return 0;
  uint32_t mode = 0;
  for (uint64_t p = s; a[p] != ' '; p++) mode = (mode << 3) + (uint32_t)(a[p] - '0');
  return canon_mode(mode);
}
// where the name begins: behind the space that ends the mode (the entry is well formed)
MD_PD_FN uint32_t entry_name(const uint8_t *a, uint32_t s) {
  while (a[s] != ' ') s++;
  return s + 1;
}

// An entry's key is its name with '/' appended iff it is a directory; keys compare bytewise, a proper prefix first.
// < 0, 0, > 0 as x's key sorts in front of, with, behind y's.
MD_PD_FN int key_compare(const uint8_t *x, const Entry &ex, const uint8_t *y, const Entry &ey) {
  const uint32_t nx = ex.nul - ex.name, ny = ey.nul - ey.name;
  const uint32_t lx = nx + (is_dir(ex.mode) ? 1u : 0u), ly = ny + (is_dir(ey.mode) ? 1u : 0u);
  const uint32_t l = lx < ly ? lx : ly;
  for (uint32_t k = 0; k < l; k++) {
    const uint32_t cx = k < nx ? x[ex.name + k] : (uint32_t)'/', cy = k < ny ? y[ey.name + k] : (uint32_t)'/';
    if (cx != cy) return cx < cy ? -1 : 1;
  }
  return lx < ly ? -1 : lx > ly ? 1 : 0;
}

// The row of y's n rows (keys strictly ascending) whose key is x's and which is a directory iff x is one, or kNone.
// rows(j): row j of y.
template <class Rows>
MD_PD_FN uint32_t find_key(const uint8_t *x, const Entry &ex, const uint8_t *y, Rows rows, uint32_t n) {
  uint32_t lo = 0, hi = n;  // the first row whose key is not in front of x's
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (key_compare(y, rows(mid), x, ex) < 0) lo = mid + 1;
    else hi = mid;
  }
  if (lo == n) return kNone;
  const Entry ey = rows(lo);
  return key_compare(y, ey, x, ex) == 0 && is_dir(ey.mode) == is_dir(ex.mode) ? lo : kNone;
}

MD_PD_FN bool same_name20(const uint8_t *x, const uint8_t *y) {
  bool same = true;
  for (uint32_t k = 0; k < 20; k++) same = same && x[k] == y[k];
  return same;
}

// What an entry of A gives: found = B holds its key (then mb and same20 are that entry's), 0 = nothing
MD_PD_FN uint32_t classify(bool found, uint32_t ma, uint32_t mb, bool same20) {
  if (!found) return 'D';
  if (is_dir(ma)) return same20 ? 0u : (uint32_t)'M';
  if (ma == mb && same20) return 0;
  return ((ma ^ mb) & 0170000) != 0 ? (uint32_t)'T' : (uint32_t)'M';
}

}  // namespace pd
}  // namespace md
