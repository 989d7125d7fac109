// pack_write.hpp — the host's arithmetic of md_pack_delta_batch_* and md_pack_write (mdeflate.h; capi_pack_write.cpp): the
// constants of the delta definition, the size of a base's table and where the tables of a batch's bases go, the bytes of an
// object's header and of an OFS_DELTA's distance, the rule that says which deltas are kept, the sequential walk from
// compressed lengths to offsets, and the bound.  Plain C++: no device code, no md_ctx (tests/pack_write_check.cpp drives it
// alone under the sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mdeflate.h"
#include "pack_index.hpp"

namespace md {
namespace pkw {

// ---- the delta definition ----
constexpr uint32_t kBlock = 16, kHashMul = 0x9E3779B1u, kMinBits = 10, kEmpty = 0xffffffffu;
constexpr uint32_t kMaxInsert = 127, kMaxCopy = 0x10000;  // bytes of one insert op, of one copy op

// k: the smallest integer >= kMinBits with 2^k >= 2 * blocks (blocks < 2^28: at most 29)
inline uint32_t table_bits(uint64_t blocks) {
  uint32_t k = kMinBits;
  while (((uint64_t)1 << k) < 2 * blocks) k++;
  return k;
}

// Where the tables of a batch's distinct bases go.  A base with a block gets, in the order the bases are added, the next
// run of blocks of the index launch and the next 2^bits words of the tables; a base of fewer than kBlock bytes gets no table
// (bits 0) and is no row of the index launch.
struct TablePlace {
  uint64_t table_off, first_block;
  uint32_t bits;
};
struct TableRoom {
  uint64_t blocks = 0, words = 0;  // of the bases added so far
  TablePlace add(uint64_t base_len) {
    const uint64_t nb = base_len / kBlock;
    if (nb == 0) return TablePlace{0, 0, 0};
    const TablePlace at = {words, blocks, table_bits(nb)};
    blocks += nb;
    words += (uint64_t)1 << at.bits;
    return at;
  }
};

// ---- md_pack_write ----
using pack::kPackHeader;
using pack::kPackTrailer;
constexpr uint32_t kOfsDelta = 6;
// a delta is tried for a target of at least kDeltaMinTarget bytes on a base of at least kBlock, into nt / 2 - kDeltaSlack bytes
constexpr uint64_t kDeltaMinTarget = 64, kDeltaSlack = 20;
// most bytes in front of an object's stream: a type / size varint of 32 bits of size (5) and a distance of 64 bits (10), rounded up
constexpr uint64_t kHeaderMax = 16;

inline bool delta_tried(uint64_t nb, uint64_t nt) { return nt >= kDeltaMinTarget && nb >= kBlock; }
inline uint64_t delta_cap(uint64_t nt) { return nt / 2 - kDeltaSlack; }

// room of an object's zlib stream: the encoder's blocks are dynamic ones of at most 4 096 symbols, a block's header stays
// below 300 bytes and no Huffman code of 286 symbols spends more than 8.3 bits on a literal - an eighth more, and 256
// for the short ones
inline uint64_t stream_room(uint64_t len) { return len + len / 8 + 256; }

// the type / size varint: (type << 4 | size & 15), then 7 bits at a time; returns its length (at most 10)
inline uint32_t object_header(uint32_t type, uint64_t size, uint8_t out[10]) {
  uint32_t k = 0;
  uint32_t c = (type << 4) | (uint32_t)(size & 15);
  size >>= 4;
  while (size) {
    out[k++] = (uint8_t)(c | 0x80);
    c = (uint32_t)(size & 0x7f);
    size >>= 7;
  }
  out[k++] = (uint8_t)c;
  return k;
}

// an OFS_DELTA's distance v >= 1, most significant group first, every group but the last one less than it says; returns its
// length (at most 10)
inline uint32_t ofs_varint(uint64_t v, uint8_t out[10]) {
  uint8_t tmp[10];
  uint32_t k = 0;
  tmp[k++] = (uint8_t)(v & 0x7f);
  while (v >>= 7) tmp[k++] = (uint8_t)(0x80 | (--v & 0x7f));
  for (uint32_t i = 0; i < k; i++) out[i] = tmp[k - 1 - i];
  return k;
}

// Which deltas are kept, in index order.  base[i]: an earlier index or MD_PACK_NO_BASE; tried[i] != 0: a delta was made for
// i; fitted[i] != 0: it fitted its room.  A delta is kept iff it fitted and its chain of kept deltas stays within
// max_depth (0: no limit); an object whose delta is dropped is written whole and counts as depth 0 for what hangs off it.
struct Kept {
  uint64_t kept = 0, dropped_size = 0, dropped_depth = 0;
};
inline Kept keep_rule(size_t n, const uint64_t *base, const uint8_t *tried, const uint8_t *fitted, uint32_t max_depth, uint8_t *keep,
                      uint32_t *depth) {
  Kept r;
  for (size_t i = 0; i < n; i++) {
    keep[i] = 0, depth[i] = 0;
    if (!tried[i]) continue;
    if (!fitted[i]) {
      r.dropped_size++;
      continue;
    }
    const uint32_t d = depth[base[i]] + 1;  // (base[i] < i: the call's check)
    if (max_depth && d > max_depth) {
      r.dropped_depth++;
      continue;
    }
    keep[i] = 1, depth[i] = d;
    r.kept++;
  }
  return r;
}

// The walk: object i stands at offset[i], its header bytes at head + kHeaderMax * i (head_len[i] of them), its stream of
// zlen[i] bytes behind them; offset[n] = where the trailer goes.  The length of a kept delta's distance depends on the
// offsets in front of it, so this is sequential.  size[i]: what the header states - the delta's length for a kept delta,
// else the content's.
inline void walk_offsets(size_t n, const uint32_t *type, const uint64_t *size, const uint64_t *base, const uint8_t *keep, const uint64_t *zlen,
                         uint64_t *offset, uint8_t *head, uint8_t *head_len) {
  uint64_t at = kPackHeader;
  for (size_t i = 0; i < n; i++) {
    uint8_t *h = head + kHeaderMax * i;
    uint8_t tmp[10];
    uint32_t k = object_header(keep[i] ? kOfsDelta : type[i], size[i], tmp);
    for (uint32_t b = 0; b < k; b++) h[b] = tmp[b];
    if (keep[i]) {
      const uint32_t m = ofs_varint(at - offset[base[i]], tmp);
      for (uint32_t b = 0; b < m && k + b < kHeaderMax; b++) h[k + b] = tmp[b];
      k += m;  // (5 + 10 at the most: below kHeaderMax)
    }
    offset[i] = at;
    head_len[i] = (uint8_t)k;
    at += k + zlen[i];
  }
  offset[n] = at;
}

// room that always suffices for the pack of objects of these lengths; 0 when it does not fit 64 bits
inline uint64_t write_bound(size_t n, const md_pack_source *objs) {
  uint64_t sum = kPackHeader + kPackTrailer;
  for (size_t i = 0; i < n; i++) {
    if (objs[i].len > MD_MAX_STREAM) return 0;
    const uint64_t one = kHeaderMax + stream_room(objs[i].len);
    if (sum > UINT64_MAX - one) return 0;
    sum += one;
  }
  return sum;
}

}  // namespace pkw
}  // namespace md
