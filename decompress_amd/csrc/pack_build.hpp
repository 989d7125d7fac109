// pack_build.hpp — the host's two parts of md_pack_index_build (mdeflate.h; capi_pack_build.cpp): the walk that finds where
// every object of a pack begins when there is no idx, and the writer of an idx version 2 (md_pack_index_write, the inverse
// of pack_index.hpp's reader).  Plain C++: no device code, no md_ctx.
//
// The walk.  The device has looked at every position z of the pack whose two bytes pass the decoder's test of a zlib
// header (pack_build_kernels.hip) and has run the size query over all of them, so the host holds, in ascending order of z,
// what a stream that began there would consume.  From byte 12 the walk parses the object header it stands on - that gives
// the stream's z -, finds z among the candidates (both ascend: one forward merge, O(C + n)) and steps to z + consumed.
// A candidate that is no object's stream is never looked at: the chain from byte 12 is a function of the pack's bytes.
// No entry of the table is trusted beyond what the walk checks itself: a z that is no candidate, a count that failed or
// a stream that would pass the trailer all end the walk.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mdeflate.h"
#include "pack_index.hpp"
#include "sha1_host.hpp"

namespace md {
namespace pkb {

using pack::kPackHeader;
using pack::kPackTrailer;
// a candidate needs this many bytes in front of the trailer (no zlib stream is shorter)
constexpr uint64_t kCandidateMin = 6;

// the test of open_stream's ZLIB branch (inflate_wave_core.hpp), no narrower and no wider
inline bool zlib_start(uint32_t cmf, uint32_t flg) { return ((cmf << 8) + flg) % 31 == 0 && (cmf & 0xf) == 8; }

// The header of the object at pack[at ..) with `end` as the bound no header may pass: type, the size it states, and z,
// where its zlib stream begins.  The rules are pk::headers_kernel's.  False: no z can be told (type 0 or 5, a size
// varint beyond 64 bits, an OFS_DELTA distance beyond 2^63, a header that passes the end).  What an OFS_DELTA's distance
// says is the table's to judge, not the walk's.
inline bool object_header(const uint8_t *pack, uint64_t at, uint64_t end, uint32_t *type, uint64_t *hsize, uint64_t *z) {
  uint64_t p = at;
  if (p >= end) return false;
  uint32_t c = pack[p++];
  const uint32_t t = (c >> 4) & 7;
  uint64_t size = c & 15;
  for (uint32_t shift = 4; c & 0x80; shift += 7) {
    if (p >= end) return false;
    c = pack[p++];
    const uint64_t b = c & 0x7f;
    if (shift >= 64 ? b != 0 : (shift > 57 && (b >> (64 - shift)) != 0)) return false;
    if (shift < 64) size |= b << shift;
  }
  if (t == 0 || t == 5) return false;
  if (t == 6) {
    uint64_t v = 0;
    c = 0x80;
    for (bool first = true; c & 0x80; first = false) {
      if (p >= end || (v >> 56) != 0) return false;
      c = pack[p++];
      v = ((first ? 0 : v + 1) << 7) | (c & 0x7f);
    }
  } else if (t == 7) {
    if (end - p < 20) return false;
    p += 20;
  }
  *type = t, *hsize = size, *z = p;
  return true;
}

// the candidates' table as the device left it: C entries, z ascending
struct Candidates {
  size_t C = 0;
  const uint64_t *z = nullptr, *consumed = nullptr, *out_len = nullptr;
  const int32_t *status = nullptr;
};

struct Walk {
  std::vector<uint64_t> off, inflated;  // per object, pack order: where it begins, what its stream inflates to
  uint64_t bad_offset = MD_PACK_NO_BASE;
  int32_t bad_status = MD_OK;
};

// MD_OK: w->off holds the `count` objects the pack's header states, the last one ends exactly on pack_len - 20.
// MD_INVALID_PACK: the walk stopped at w->bad_offset (w->bad_status: the count's status if that is what stopped it).
// pack_len >= 32 is the caller's check.
inline int walk(const uint8_t *pack, uint64_t pack_len, const Candidates &c, Walk *w) {
  const uint64_t end = pack_len - kPackTrailer, count = pack::be32(pack + 8);
  uint64_t at = kPackHeader;
  size_t k = 0;
  const auto stop = [&](uint64_t where, int32_t st) {
    w->bad_offset = where, w->bad_status = st;
    return MD_INVALID_PACK;
  };
  while (at < end) {
    if (w->off.size() == count) return stop(at, MD_OK);  // more than the header states, or bytes in front of the trailer
    uint32_t type = 0;
    uint64_t hsize = 0, z = 0;
    if (!object_header(pack, at, end, &type, &hsize, &z)) return stop(at, MD_OK);
    while (k < c.C && c.z[k] < z) k++;
    if (k == c.C || c.z[k] != z) return stop(at, MD_OK);
    if (c.status[k] != MD_OK) return stop(at, c.status[k]);
    if (c.consumed[k] > end - z) return stop(at, MD_OK);  // (never, of a count that was given end - z bytes)
    w->off.push_back(at);
    w->inflated.push_back(c.out_len[k]);
    at = z + c.consumed[k];
  }
  if (w->off.size() != count) return stop(end, MD_OK);
  return MD_OK;
}

inline void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }

// the length of the idx of n objects of which m have an offset above 0x7fffffff
inline uint64_t index_len(uint64_t n, uint64_t m) { return pack::kIdxHeader + pack::kIdxFan + 28 * n + 8 * m + pack::kIdxTrailer; }

// The idx of `n` entries in any order: sorted by name here (two equal names: MD_INVALID_INDEX), offsets above 0x7fffffff
// through the 64-bit table in idx order, then the pack's checksum and the idx's own SHA-1.  *idx_len: the idx's length,
// also when idx_cap is too small for it (MD_UNEXPECTED_END_OF_OUTPUT, nothing written).
inline int write_index(const md_pack_index_entry *e, size_t n, const uint8_t pack_checksum[20], uint8_t *idx, size_t idx_cap, size_t *idx_len) {
  *idx_len = 0;
  if (n > 0xffffffffull) return MD_E_INVALID_ARGUMENT;  // (the fan-out's words are 32-bit)
  std::vector<uint32_t> order(n);
  uint64_t m = 0;
  for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i, m += e[i].offset > 0x7fffffffull;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const int c = memcmp(e[a].name, e[b].name, pack::kName);
    return c != 0 ? c < 0 : a < b;
  });
  for (size_t s = 1; s < n; s++)
    if (memcmp(e[order[s - 1]].name, e[order[s]].name, pack::kName) == 0) return MD_INVALID_INDEX;
  const uint64_t len = index_len(n, m);
  *idx_len = (size_t)len;
  if (len > idx_cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  put32(idx, 0xff744f63u), put32(idx + 4, 2);
  uint32_t fan[256] = {0};
  for (size_t i = 0; i < n; i++) fan[e[i].name[0]]++;
  uint32_t run = 0;
  for (int b = 0; b < 256; b++) run += fan[b], put32(idx + pack::kIdxHeader + 4 * b, run);
  uint8_t *names = idx + pack::kIdxHeader + pack::kIdxFan, *crcs = names + n * pack::kName, *offs = crcs + n * 4, *big = offs + n * 4;
  uint32_t escaped = 0;
  for (size_t s = 0; s < n; s++) {
    const md_pack_index_entry &o = e[order[s]];
    memcpy(names + s * pack::kName, o.name, pack::kName);
    put32(crcs + 4 * s, o.crc32);
    if (o.offset > 0x7fffffffull) {
      put32(offs + 4 * s, 0x80000000u | escaped);
      put32(big + 8 * (size_t)escaped, (uint32_t)(o.offset >> 32)), put32(big + 8 * (size_t)escaped + 4, (uint32_t)o.offset);
      escaped++;
    } else {
      put32(offs + 4 * s, (uint32_t)o.offset);
    }
  }
  uint8_t *tail = big + 8 * m;
  memcpy(tail, pack_checksum, pack::kName);
  sha::sha1_of(idx, (size_t)(tail + pack::kName - idx), tail + pack::kName);
  return MD_OK;
}

}  // namespace pkb
}  // namespace md
