// gz_rfc.hpp — the header of one GZip member as RFC 1952 defines it and libz reads it, for the many-member entry points
// (md_gz_members_*, md_bgzf_*): gz_members.hip runs it per member on the device, capi.cpp on the host for files without
// a size index.  NOT Gz.Inf's reading (gz_kernels.hip keeps the reference's: FEXTRA's length big-endian, the header CRC
// the upper half of a CRC-32 that skips the extra field): here XLEN is little-endian, CM must be 8, the reserved flag
// bits must be clear, and FHCRC is the low 16 bits of the CRC-32 of every header byte in front of it, little-endian.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdeflate.h"

namespace md {
namespace gz {

__host__ __device__ inline uint32_t rfc_crc_byte(uint32_t c, uint32_t b) {
  c ^= b;
  for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1)));
  return c;
}

// s[0, len): what is left of the file from the member's first byte on.  MD_OK: *hdr_len = bytes in front of the body.
__host__ __device__ inline int rfc_header(const uint8_t *s, uint64_t len, uint64_t *hdr_len) {
  *hdr_len = 0;
  // what is there decides before what is missing: two bytes of garbage are a bad header, not a short one
  if ((len >= 1 && s[0] != 0x1f) || (len >= 2 && s[1] != 0x8b) || (len >= 3 && s[2] != 8) || (len >= 4 && (s[3] & 0xe0)))
    return MD_INVALID_GZIP_HEADER;
  if (len < 10) return MD_UNEXPECTED_END_OF_INPUT;
  const uint32_t flg = s[3];
  uint64_t p = 10;
  if (flg & 4) {
    if (len - p < 2) return MD_UNEXPECTED_END_OF_INPUT;
    const uint64_t xl = (uint64_t)s[p] | ((uint64_t)s[p + 1] << 8);
    p += 2;
    if (len - p < xl) return MD_UNEXPECTED_END_OF_INPUT;
    p += xl;
  }
  for (int which = 0; which < 2; which++) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & (which == 0 ? 8u : 16u))) continue;
    for (;;) {
      if (p >= len) return MD_UNEXPECTED_END_OF_INPUT;
      if (s[p++] == 0) break;
    }
  }
  if (flg & 2) {
    if (len - p < 2) return MD_UNEXPECTED_END_OF_INPUT;
    uint32_t crc = 0xffffffffu;
    for (uint64_t k = 0; k < p; k++) crc = rfc_crc_byte(crc, s[k]);
    const uint32_t want = (crc ^ 0xffffffffu) & 0xffffu, have = (uint32_t)s[p] | ((uint32_t)s[p + 1] << 8);
    if (want != have) return MD_INVALID_GZIP_HEADER_CHECKSUM;
    p += 2;
  }
  *hdr_len = p;
  return MD_OK;
}

}  // namespace gz
}  // namespace md
