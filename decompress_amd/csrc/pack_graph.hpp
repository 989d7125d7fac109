// pack_graph.hpp — how a commit, a tree and a tag name other objects (md_pack_graph_build; the rules are mdeflate.h's, read
// off git's decode_tree_entry, parse_commit_buffer and parse_tag_buffer).  The rules live here once: the link kernels
// (pack_graph_kernels.hip) and the host check of the tests (tests/pack_graph_check.cpp) run these very functions.  Plain C++
// with no HIP in it: a host compiler alone takes it; under hipcc the functions are the device's too.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MD_PG_FN __host__ __device__ inline
#else
#define MD_PG_FN inline
#endif

namespace md {
namespace pg {

constexpr uint32_t kNoLink = 0xffffffffu;  // MD_PACK_NO_LINK
// an edge's kind (the low bits) and its two flags
constexpr uint32_t kCommitTree = 1, kCommitParent = 2, kTagTarget = 3, kTreeBlob = 4, kTreeTree = 5, kTreeGitlink = 6;
constexpr uint32_t kAbsent = 0x40, kMistyped = 0x80;
constexpr uint32_t kMalformed = 0;  // what a parse function returns for an object whose links cannot be read

constexpr uint64_t kNameBytes = 20, kHexBytes = 40;
// the shortest tree entry: a mode digit, the space, one byte of name, the NUL, the 20 bytes
constexpr uint64_t kMinEntry = 24;
constexpr uint64_t kTreeLine = 46, kParentLine = 48;  // "tree " + 40 + '\n'; "parent " + 40 + '\n'

// most edges an object of `size` bytes and type 1, 2 or 4 can have: what its slot holds before the edges are compacted
MD_PG_FN uint64_t edge_bound(uint32_t type, uint64_t size) {
  if (type == 2) return size / kMinEntry;
  if (type == 1) return size >= kTreeLine ? 1 + (size - kTreeLine) / kParentLine : 0;
  return type == 4 ? 1 : 0;
}

// the type an edge's target has to have (1 commit, 2 tree, 3 blob, 4 tag); tag_type: what a tag's type line states
MD_PG_FN uint32_t wanted_type(uint32_t kind, uint32_t tag_type) {
  return kind == kCommitTree || kind == kTreeTree ? 2 : kind == kCommitParent ? 1 : kind == kTreeBlob ? 3 : kind == kTagTarget ? tag_type : 0;
}

// the flag of an edge whose name was looked up: found = it is among the pack's names, type = that object's (0: not known)
MD_PG_FN uint32_t edge_flag(bool found, uint32_t type, uint32_t wanted) {
  if (!found) return kAbsent;
  return type >= 1 && type <= 4 && type != wanted ? kMistyped : 0;
}

// ---- trees ----
// A tree of `size` bytes whose last 21 begin with the byte last21 is walked at all (an empty one has no entry and is sound)
MD_PG_FN bool tree_walkable(uint64_t size, uint32_t last21) { return size >= kMinEntry - 1 && last21 == 0; }

// The entry that starts at a[s] and whose name ends with the NUL at a[nul], the first NUL at or behind s (the caller has
// it from the chain; s <= nul): its kind by git's canon_mode, or kMalformed - an empty mode, a byte other than '0'..'7' in
// front of the space, no space, an empty name.  Reads a[s .. nul] alone.  The 20 bytes behind the NUL are the target's name.
MD_PG_FN uint32_t tree_entry_kind(const uint8_t *a, uint64_t s, uint64_t nul) {
  uint32_t mode = 0;
  uint64_t p = s;
  if (a[p] == ' ') return kMalformed;
  for (;; p++) {  // (the NUL at a[nul] is no digit: the loop ends there at the latest)
    const uint32_t c = a[p];
    if (c == ' ') break;
    if (c < '0' || c > '7') return kMalformed;
    mode = (mode << 3) + (c - '0');
  }
  if (p + 1 == nul) return kMalformed;
  const uint32_t fmt = mode & 0170000;
  return fmt == 0100000 || fmt == 0120000 ? kTreeBlob : fmt == 0040000 ? kTreeTree : kTreeGitlink;
}

// One tree from its first byte to its last, entry by entry - the chain the tree kernel follows a window at a time:
// emit(position, kind, the 20 name bytes) for every entry; false: the tree is malformed (whatever was emitted does not count)
template <class Emit>
MD_PG_FN bool tree_walk(const uint8_t *a, uint64_t size, Emit emit) {
  if (size == 0) return true;
  if (!tree_walkable(size, size >= kNameBytes + 1 ? a[size - kNameBytes - 1] : 1)) return false;
  uint64_t pos = 0;
  for (uint64_t s = 0; s < size; pos++) {
    if (size - s < kMinEntry - 1) return false;
    uint64_t nul = s;
    while (a[nul] != 0) nul++;  // (a[size - 21] is one)
    const uint32_t kind = tree_entry_kind(a, s, nul);
    if (kind == kMalformed || nul + 1 + kNameBytes > size) return false;
    emit(pos, kind, a + nul + 1);
    s = nul + 1 + kNameBytes;
  }
  return true;
}

// ---- commits and tags ----
MD_PG_FN int hex_digit(uint32_t c) {
  return c >= '0' && c <= '9' ? (int)c - '0' : c >= 'a' && c <= 'f' ? (int)c - 'a' + 10 : c >= 'A' && c <= 'F' ? (int)c - 'A' + 10 : -1;
}
MD_PG_FN bool hex_name(const uint8_t *h) {  // 40 hex digits of either case
  bool ok = true;
  for (uint64_t k = 0; k < kHexBytes; k++) ok = ok && hex_digit(h[k]) >= 0;
  return ok;
}
// byte k of the name that the 40 digits at h spell (hex_name(h) holds)
MD_PG_FN uint32_t hex_byte(const uint8_t *h, uint32_t k) { return (uint32_t)(hex_digit(h[2 * k]) << 4 | hex_digit(h[2 * k + 1])); }

MD_PG_FN bool starts(const uint8_t *a, const char *word, uint64_t n) {
  bool ok = true;
  for (uint64_t k = 0; k < n; k++) ok = ok && a[k] == (uint8_t)word[k];
  return ok;
}

// A commit: emit(position, kind, where the name's 40 hex digits stand) for its tree and then every parent line that
// follows; false: malformed.  Nothing behind the parent lines is read.
template <class Emit>
MD_PG_FN bool commit_walk(const uint8_t *a, uint64_t size, Emit emit) {
  if (size <= kTreeLine || !starts(a, "tree ", 5) || !hex_name(a + 5) || a[kTreeLine - 1] != '\n') return false;
  emit((uint64_t)0, kCommitTree, a + 5);
  uint64_t pos = 1;
  for (uint64_t p = kTreeLine; p + kParentLine - 1 < size && starts(a + p, "parent ", 7); p += kParentLine, pos++) {
    if (size <= p + kParentLine || !hex_name(a + p + 7) || a[p + kParentLine - 1] != '\n') return false;
    emit(pos, kCommitParent, a + p + 7);
  }
  return true;
}

// A tag: the type its type line states (1 .. 4) with the target's 40 hex digits at a + 7, or 0: malformed
MD_PG_FN uint32_t tag_target_type(const uint8_t *a, uint64_t size) {
  if (size < 64 || !starts(a, "object ", 7) || !hex_name(a + 7) || a[47] != '\n' || !starts(a + 48, "type ", 5)) return 0;
  const uint8_t *t = a + 53;  // (the longest type name and its newline end at byte 60)
  uint32_t type = 0;
  uint64_t p = 0;
  if (starts(t, "commit\n", 7)) type = 1, p = 60;
  else if (starts(t, "tree\n", 5)) type = 2, p = 58;
  else if (starts(t, "blob\n", 5)) type = 3, p = 58;
  else if (starts(t, "tag\n", 4)) type = 4, p = 57;
  if (type == 0 || !(p + 4 < size) || !starts(a + p, "tag ", 4)) return 0;
  return type;
}

}  // namespace pg
}  // namespace md
