// bgzf_index.hpp — the index of a blocked GZip file (BGZF: bgzip, htslib, .bam, .vcf.gz; mdeflate.h: md_bgzf_index_*):
// where every member begins in the file and in its output, and the .gzi form of that table.  Plain C++: no device code,
// no md_ctx.  The .gzi layout is written from htslib's description of it (a little-endian u64 count N, then N pairs of
// u64 (compressed offset, uncompressed offset), the first block (0, 0) not stored); nobody here could run htslib against
// it.  `from_gzi` checks everything a later read trusts, and reads no byte of the blob or of src before it has checked
// that the byte is there.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <new>
#include <vector>

#include "mdeflate.h"

// M members: c_off / u_off hold M + 1 entries, both begin with 0; member k is src[c_off[k], c_off[k + 1]) and its output
// [u_off[k], u_off[k + 1]).  c_off[M] is the byte behind the last member (<= src_len: NUL padding may follow).
struct md_bgzf_index {
  uint64_t src_len = 0;
  std::vector<uint64_t> c_off{0}, u_off{0};
  size_t members() const { return c_off.size() - 1; }
  uint64_t size() const { return u_off.back(); }
};

namespace md {
namespace bgzf {

// most output a member of `len` bytes can have: no DEFLATE stream yields more than 1 032 bytes per byte of input
constexpr uint64_t kMaxExpansion = 1032;

inline uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }
inline uint64_t rd64(const uint8_t *p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }
inline void wr64(uint8_t *p, uint64_t v) {
  for (int k = 0; k < 8; k++) p[k] = (uint8_t)(v >> (8 * k));
}

// Length of the indexed member that starts at src[p] (p < len), 0 if none does: 1f 8b 08, FLG with FEXTRA and no reserved
// bit, and in the extra field a subfield 'B' 'C' of length 2 whose BSIZE + 1 is a member length that fits the header and
// ends inside src - the member scan's rule (gz_members.hip: indexed_member_at), on the host.
inline uint32_t member_at(const uint8_t *src, uint64_t len, uint64_t p) {
  if (len - p < 12 + 6 + 2 + 8) return 0;
  const uint8_t *h = src + p;
  if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0xe4) != 4) return 0;
  const uint32_t xlen = rd16(h + 10);
  if (len - p - 12 < xlen) return 0;
  for (uint32_t q = 0; q + 4 <= xlen;) {
    const uint8_t *f = h + 12 + q;
    const uint32_t sl = rd16(f + 2);
    if (q + 4 + sl > xlen) return 0;
    if (f[0] == 'B' && f[1] == 'C' && sl == 2) {
      const uint32_t m = rd16(f + 4) + 1;
      return m < 12 + xlen + 2 + 8 || m > len - p ? 0 : m;
    }
    q += 4 + sl;
  }
  return 0;
}

inline size_t gzi_size(const md_bgzf_index *x) { return 8 + 16 * (x->members() > 1 ? x->members() - 1 : 0); }

// members 1 .. M - 1 (buf holds gzi_size(x) bytes)
inline void to_gzi(const md_bgzf_index *x, uint8_t *buf) {
  const size_t M = x->members(), N = M > 1 ? M - 1 : 0;
  wr64(buf, N);
  for (size_t k = 1; k <= N; k++) {
    wr64(buf + 8 + 16 * (k - 1), x->c_off[k]);
    wr64(buf + 16 + 16 * (k - 1), x->u_off[k]);
  }
}

// MD_OK and *res (the caller's to delete), MD_INVALID_INDEX, or MD_E_OUT_OF_MEMORY.  The blob's rules: exactly 8 + 16 N
// bytes; compressed offsets increase strictly (from the implied 0) and are < src_len; uncompressed offsets do not
// decrease, and a member's output is at most kMaxExpansion times its length.  .gzi does not say where the file ends or how
// large its output is, so the table is completed from src: from the last entry on (offset 0 when N is 0) the BSIZE fields
// are followed member by member, each ISIZE taken from its trailer, to the end of src or to NUL padding that reaches it.
inline int from_gzi(const uint8_t *gzi, size_t gzi_len, const uint8_t *src, size_t src_len, md_bgzf_index **res) {
  *res = nullptr;
  if (gzi_len < 8) return MD_INVALID_INDEX;
  const uint64_t N = rd64(gzi);
  if (N > (gzi_len - 8) / 16 || gzi_len - 8 != 16 * N) return MD_INVALID_INDEX;  // (also bounds what is allocated)
  md_bgzf_index *x = new (std::nothrow) md_bgzf_index();
  if (!x) return MD_E_OUT_OF_MEMORY;
  int rc = MD_OK;
  try {
    x->src_len = src_len;
    x->c_off.reserve((size_t)N + 3);
    x->u_off.reserve((size_t)N + 3);
    for (uint64_t k = 0; k < N && rc == MD_OK; k++) {
      const uint64_t c = rd64(gzi + 8 + 16 * k), u = rd64(gzi + 16 + 16 * k), c0 = x->c_off.back(), u0 = x->u_off.back();
      if (c <= c0 || c >= src_len || u < u0 || (u - u0) / kMaxExpansion > c - c0) rc = MD_INVALID_INDEX;
      x->c_off.push_back(c);
      x->u_off.push_back(u);
    }
    // the walk: the entries in front of the last one get their members' word against them when they are read
    uint64_t p = x->c_off.back(), u = x->u_off.back();
    bool first = true;
    while (rc == MD_OK && p < src_len) {
      if (src[p] == 0 && !first) {  // padding: it has to reach the end
        uint64_t q = p;
        while (q < src_len && src[q] == 0) q++;
        if (q != src_len) rc = MD_INVALID_INDEX;
        break;
      }
      const uint32_t m = member_at(src, src_len, p);
      if (m == 0) {
        rc = MD_INVALID_INDEX;
        break;
      }
      const uint64_t isize = rd32(src + p + m - 4);
      if (u + isize < u) {
        rc = MD_INVALID_INDEX;
        break;
      }
      p += m;
      u += isize;
      if (first) first = false;
      else {
        x->c_off.push_back(p - m);
        x->u_off.push_back(u - isize);
      }
    }
    if (rc == MD_OK && !first) {  // the end of the last member (no member at all: an empty src, an index of 0 members)
      x->c_off.push_back(p);
      x->u_off.push_back(u);
    }
  } catch (const std::bad_alloc &) {
    rc = MD_E_OUT_OF_MEMORY;
  }
  if (rc != MD_OK) {
    delete x;
    return rc;
  }
  *res = x;
  return MD_OK;
}

}  // namespace bgzf
}  // namespace md
