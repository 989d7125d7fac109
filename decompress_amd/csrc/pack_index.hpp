// pack_index.hpp — the .idx (version 2) beside a git packfile (mdeflate.h: md_pack_index): names, CRC-32s and offsets of
// the pack's objects, in ascending order of name.  Plain C++: no device code, no md_ctx.  Written from git's description
// of the format (Documentation/gitformat-pack.txt); every number is big-endian, and no byte is read before it has been
// checked that the byte is there.
//
//   0     ff 74 4f 63, u32 version = 2
//   8     256 x u32 fan-out: fan[b] = names whose first byte is <= b; n = fan[255]
//   1032  n x 20 bytes of name, n x u32 CRC-32 of the packed object, n x u32 offset (bit 31: the low 31 bits index the
//         table that follows), m x u64 offset, 20 bytes the pack's checksum, 20 bytes the idx's own
//
// m is not stated: it is the number of entries whose bit 31 is set, and the file's length must be exactly what n and m
// give.  An idx of a SHA-256 repository (32-byte names) cannot be told apart by its header; it fails that length rule
// and ends as MD_INVALID_INDEX.  Idx version 1 has no magic: MD_PACK_UNSUPPORTED.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "mdeflate.h"

namespace md {
namespace pack {

constexpr size_t kIdxHeader = 8, kIdxFan = 1024, kIdxTrailer = 40, kName = 20;
// the pack itself: "PACK", u32 version, u32 count in front of the objects, the SHA-1 of all that behind them
constexpr uint64_t kPackHeader = 12, kPackTrailer = 20;

inline uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }
inline uint64_t be64(const uint8_t *p) { return (uint64_t)be32(p) << 32 | be32(p + 4); }

// MD_INVALID_PACK: too short for a header and a trailer, or no "PACK"; MD_PACK_UNSUPPORTED: a version that is neither 2 nor 3
inline int pack_header_status(const uint8_t *pack, size_t len) {
  if (len < kPackHeader + kPackTrailer || memcmp(pack, "PACK", 4) != 0) return MD_INVALID_PACK;
  const uint32_t version = be32(pack + 4);
  return version == 2 || version == 3 ? MD_OK : MD_PACK_UNSUPPORTED;
}

// MD_OK, MD_INVALID_INDEX or MD_PACK_UNSUPPORTED; info is filled on MD_OK, and the first min(cap, n) entries
inline int read_index(const uint8_t *idx, size_t idx_len, md_pack_index_info *info, md_pack_index_entry *entries, size_t cap) {
  memset(info, 0, sizeof *info);
  if (idx_len < kIdxHeader) return MD_INVALID_INDEX;
  if (be32(idx) != 0xff744f63u || be32(idx + 4) != 2) return MD_PACK_UNSUPPORTED;
  if (idx_len < kIdxHeader + kIdxFan + kIdxTrailer) return MD_INVALID_INDEX;
  const uint8_t *fan = idx + kIdxHeader;
  uint32_t prev = 0;
  for (int b = 0; b < 256; b++) {
    const uint32_t f = be32(fan + 4 * b);
    if (f < prev) return MD_INVALID_INDEX;
    prev = f;
  }
  const uint64_t n = prev, room = idx_len - (kIdxHeader + kIdxFan + kIdxTrailer);
  if (n > room / 28) return MD_INVALID_INDEX;  // (also bounds every product below)
  const uint8_t *names = fan + kIdxFan, *crcs = names + n * kName, *offs = crcs + n * 4, *big = offs + n * 4;
  uint64_t m = 0;
  for (uint64_t i = 0; i < n; i++) m += offs[4 * i] >> 7;
  if (room - n * 28 != m * 8) return MD_INVALID_INDEX;
  // the names: ascending strictly, each where the fan-out puts its first byte
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t *nm = names + i * kName;
    if (i && memcmp(nm - kName, nm, kName) >= 0) return MD_INVALID_INDEX;
    const uint32_t lo = nm[0] ? be32(fan + 4 * (nm[0] - 1)) : 0, hi = be32(fan + 4 * nm[0]);
    if (i < lo || i >= hi) return MD_INVALID_INDEX;
  }
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t o = be32(offs + 4 * i);
    uint64_t off = o;
    if (o >> 31) {
      if ((o & 0x7fffffffu) >= m) return MD_INVALID_INDEX;
      off = be64(big + 8 * (uint64_t)(o & 0x7fffffffu));
    }
    if (i < cap) {
      md_pack_index_entry &e = entries[i];
      e.offset = off;
      e.crc32 = be32(crcs + 4 * i);
      memcpy(e.name, names + i * kName, kName);
    }
  }
  info->n = n;
  info->has_64bit_table = m != 0;
  memcpy(info->pack_checksum, big + m * 8, kName);
  return MD_OK;
}

// the index of name20 among n entries' names (stride: bytes from one name to the next), by the fan-out; -1 if absent
inline int64_t find_name(const uint8_t *names, size_t stride, const uint32_t *fan256, const uint8_t *name20) {
  uint64_t lo = name20[0] ? fan256[name20[0] - 1] : 0, hi = fan256[name20[0]];
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const int c = memcmp(names + mid * stride, name20, kName);
    if (c == 0) return (int64_t)mid;
    if (c < 0) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

}  // namespace pack
}  // namespace md
