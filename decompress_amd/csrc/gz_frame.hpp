// gz_frame.hpp — Gz.Inf's reading of a GZip header, on the host (lib/gz.ml:463-531, as gz_header_kernel reads it for the
// batch path): FEXTRA's length is big-endian, FHCRC is the upper half of the CRC-32 of the ten fixed bytes, the name and
// the comment (the extra field is skipped), big-endian.  gz_rfc.hpp is the other reading, RFC 1952's and libz's.  Plain
// C++ without HIP or a context, as zindex.hpp and zip_dir.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "host_util.hpp"
#include "mdeflate.h"

namespace md {
namespace gz {

// where the parts of a header lie, as offsets from its first byte; a field that the flags do not announce has length 0
struct InfHeader {
  size_t body;  // the DEFLATE stream
  uint32_t flg, mtime, xfl, os;
  size_t extra_off, extra_len, name_off, name_len, comment_off, comment_len;  // (name and comment without their NUL)
};

// MD_OK and *h; MD_UNEXPECTED_END_OF_INPUT: the n bytes end inside the header; MD_INVALID_GZIP_HEADER;
// MD_INVALID_GZIP_HEADER_CHECKSUM.  The reference looks at the ID bytes only once the ten fixed bytes are there: a cut
// header of fewer bytes is "unexpected end of input" whatever its first bytes are.
inline int inf_header(const uint8_t *s, size_t n, InfHeader *h) {
  *h = InfHeader();
  if (n < 10) return MD_UNEXPECTED_END_OF_INPUT;
  if (s[0] != 0x1f || s[1] != 0x8b) return MD_INVALID_GZIP_HEADER;
  h->flg = s[3];
  h->mtime = be32(s + 4);
  h->xfl = s[8];
  h->os = s[9];
  size_t p = 10;
  if (h->flg & 4) {
    if (n - p < 2) return MD_UNEXPECTED_END_OF_INPUT;
    h->extra_len = ((size_t)s[p] << 8) | s[p + 1];
    h->extra_off = p += 2;
    if (n - p < h->extra_len) return MD_UNEXPECTED_END_OF_INPUT;
    p += h->extra_len;
  }
  const size_t after_extra = p;
  for (int which = 0; which < 2; which++) {
    if (!(h->flg & (which == 0 ? 8u : 16u))) continue;
    const size_t from = p;
    while (p < n && s[p] != 0) p++;
    if (p >= n) return MD_UNEXPECTED_END_OF_INPUT;
    (which == 0 ? h->name_off : h->comment_off) = from;
    (which == 0 ? h->name_len : h->comment_len) = p - from;
    p++;
  }
  if (h->flg & 2) {
    if (n - p < 2) return MD_UNEXPECTED_END_OF_INPUT;
    const uint32_t c = crc32_update(crc32_update(0, s, 10), s + after_extra, p - after_extra);
    if ((c >> 16) != (((uint32_t)s[p] << 8) | s[p + 1])) return MD_INVALID_GZIP_HEADER_CHECKSUM;
    p += 2;
  }
  h->body = p;
  return MD_OK;
}

}  // namespace gz
}  // namespace md
