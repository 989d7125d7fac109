// host_util.hpp — small host-side helpers of capi*.cpp and stream_*.cpp: checksums of the few bytes the host
// handles itself, 32-bit reads of header and trailer fields, the carver that splits one block of memory into arrays, the
// running sum of output offsets and the walk over the ranges that leave by one copy.  Plain C++ without HIP: a host
// compiler alone takes it (gz_frame.hpp and the sanitizer programs of tests/ do).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace md {

// a 32-bit field of a frame: little-endian (GZip's trailer) / big-endian (ZLIB's)
inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// Adler-32 going on from `adler` (lib/de.ml:4217-4218 keeps it per fill; the sum is the same)
inline uint32_t adler32_update(uint32_t adler, const uint8_t *p, size_t n) {
  uint32_t a = adler & 0xffff, b = adler >> 16;
  while (n) {
    size_t k = n < 5552 ? n : 5552;
    n -= k;
    while (k--) {
      a += *p++;
      b += a;
    }
    a %= 65521u;
    b %= 65521u;
  }
  return (b << 16) | a;
}

// CRC-32 going on from `crc` (a complete value: 0 for none yet), eight bytes a step
struct Crc32Tables {
  uint32_t t[8][256];
  Crc32Tables() {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1)));
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; i++)
      for (int j = 1; j < 8; j++) t[j][i] = (t[j - 1][i] >> 8) ^ t[0][t[j - 1][i] & 0xff];
  }
};
inline uint32_t crc32_update(uint32_t crc, const uint8_t *p, size_t n) {
  static const Crc32Tables T;
  uint32_t c = ~crc;
  while (n >= 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = T.t[7][lo & 0xff] ^ T.t[6][(lo >> 8) & 0xff] ^ T.t[5][(lo >> 16) & 0xff] ^ T.t[4][lo >> 24] ^ T.t[3][hi & 0xff] ^
        T.t[2][(hi >> 8) & 0xff] ^ T.t[1][(hi >> 16) & 0xff] ^ T.t[0][hi >> 24];
    p += 8;
    n -= 8;
  }
  while (n--) c = T.t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
  return ~c;
}

// crc(A || B) = crc(A) * x^(8|B|) mod P xor crc(B) in GF(2)[x] / P, reflected (bit 31 = x^0): the CRC-32 of output
// whose pieces' CRCs came from the device
inline uint32_t crc32_gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; k++) {
    p ^= b & (0u - ((a >> 31) & 1));
    a <<= 1;
    b = (b >> 1) ^ (0xedb88320u & (0u - (b & 1)));
  }
  return p;
}
inline uint32_t crc32_concat(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  uint32_t sq = 0x00800000u, r = 0x80000000u;  // x^8, x^0
  for (uint64_t n = len_b; n; n >>= 1) {
    if (n & 1) r = crc32_gf_mul(r, sq);
    sq = crc32_gf_mul(sq, sq);
  }
  return crc32_gf_mul(crc_a, r) ^ crc_b;
}

// One block of memory split into arrays, every array on 16 bytes from the block's start.  Over a null base it hands out
// null pointers and only counts: `at` is then the size of the block that a second carver, over the block itself, splits
// in the same way.
struct Carver {
  uint8_t *p;
  size_t at = 0;
  explicit Carver(void *base = nullptr) : p((uint8_t *)base) {}
  template <class T>
  T *take(size_t n) {
    T *r = p ? (T *)(p + at) : nullptr;
    at += (n * sizeof(T) + 15) & ~(size_t)15;
    return r;
  }
};

// out_off[0 .. k] = the running sum of size_of(0 .. k - 1); returns the total.  A sum above 64 bits stays UINT64_MAX from
// there on, which no buffer holds.
template <class SizeOf>
uint64_t running_offsets(size_t k, uint64_t *out_off, SizeOf size_of) {
  uint64_t at = 0;
  for (size_t j = 0; j < k; j++) {
    out_off[j] = at;
    const uint64_t sz = size_of(j);
    at = at + sz < at ? UINT64_MAX : at + sz;
  }
  return out_off[k] = at;
}

// The copy-out of n ranges: f(first, bytes) once per longest run of consecutive ranges that succeeded (status 0), have
// bytes and are adjacent in dst - what is adjacent there leaves by one copy.  A failed range and a range of no bytes are
// skipped and end the run in front of them.  Stops at the first f that does not return 0 and returns that.
template <class F>
int adjacent_runs(size_t n, const int32_t *status, const uint64_t *len, const uint64_t *dst_off, F f) {
  for (size_t i = 0; i < n;) {
    if (status[i] != 0 || len[i] == 0) {
      i++;
      continue;
    }
    size_t e = i + 1;
    uint64_t bytes = len[i];
    while (e < n && status[e] == 0 && len[e] && dst_off[e] == dst_off[i] + bytes) bytes += len[e++];
    const int rc = f(i, bytes);
    if (rc != 0) return rc;
    i = e;
  }
  return 0;
}

}  // namespace md
