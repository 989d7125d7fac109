// sha1_host.hpp — SHA-1 (FIPS 180-4) as the library uses it for git object names: the block step and the formatter of a git
// object's header, both written once for the host and for the kernel of sha1_kernels.hip, and a plain host SHA-1 (init /
// update / final) for the pack's and the idx's trailers (md_pack_check_trailers) and as the kernel's CPU twin in the tests.
// No HIP in it: the two shared functions carry __host__ __device__ only where a HIP compiler reads them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MD_SHA_HD __host__ __device__
#else
#define MD_SHA_HD
#endif
#if defined(__clang__)
#define MD_SHA_UNROLL _Pragma("unroll")
#else
#define MD_SHA_UNROLL _Pragma("GCC unroll 80")
#endif
#ifndef __has_builtin
#define __has_builtin(x) 0
#endif

namespace md {
namespace sha {

// the types of a message: 0 = the bytes as they are, 1 .. 4 = a git object of that type ("<type> <size>\0" goes in front)
constexpr uint32_t kPlain = 0, kMaxType = 4;
constexpr uint32_t kHeaderMax = 18;  // "commit 4294967280\0"
constexpr uint32_t kHeaderWords = 5;

MD_SHA_HD inline uint32_t rotl(uint32_t x, uint32_t n) {
#if __has_builtin(__builtin_rotateleft32)
  return __builtin_rotateleft32(x, n);
#else
  return (x << n) | (x >> (32 - n));
#endif
}

MD_SHA_HD inline void init(uint32_t h[5]) {
  h[0] = 0x67452301u, h[1] = 0xefcdab89u, h[2] = 0x98badcfeu, h[3] = 0x10325476u, h[4] = 0xc3d2e1f0u;
}

// One block: w holds its 16 big-endian words and is the schedule's ring (it is overwritten).  Every index is a constant
// once the loop is unrolled, so on the device h and w stay in registers.
MD_SHA_HD inline void block(uint32_t h[5], uint32_t w[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
  MD_SHA_UNROLL
  for (int t = 0; t < 80; t++) {
    uint32_t wt = w[t & 15];
    if (t >= 16) {
      wt = rotl(w[(t - 3) & 15] ^ w[(t - 8) & 15] ^ w[(t - 14) & 15] ^ wt, 1);
      w[t & 15] = wt;
    }
    uint32_t f, k;
    if (t < 20) f = (b & c) | (~b & d), k = 0x5a827999u;
    else if (t < 40) f = b ^ c ^ d, k = 0x6ed9eba1u;
    else if (t < 60) f = (b & c) | (b & d) | (c & d), k = 0x8f1bbcdcu;
    else f = b ^ c ^ d, k = 0xca62c1d6u;
    const uint32_t tmp = rotl(a, 5) + f + e + k + wt;
    e = d, d = c, c = rotl(b, 30), b = a, a = tmp;
  }
  h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e;
}

// hw |= the 12 bytes of d (three big-endian words) moved S bytes down the header.  S is a constant, so every word index is
// one too: on the device nothing here is an array addressed by a variable, which would live in scratch memory.
template <uint32_t S>
MD_SHA_HD inline void header_place(const uint32_t d[3], uint32_t hw[kHeaderWords]) {
  constexpr int ws = S / 4, bs = 8 * (S % 4);
  MD_SHA_UNROLL
  for (int i = 0; i < (int)kHeaderWords; i++) {
    const int k = i - ws;
    if (k >= 0 && k < 3) hw[i] |= d[k] >> bs;
    if (bs != 0 && k >= 1 && k < 4) hw[i] |= d[k - 1] << ((32 - bs) & 31);
  }
}

// The header of a git object of `type` (1 commit, 2 tree, 3 blob, 4 tag) and `size` bytes: "<type> <size in decimal>\0",
// as the first bytes of the message's big-endian words, zeros behind it.  Returns its length, 6 .. 18; 0 (and no bytes)
// for kPlain or a type above kMaxType.
MD_SHA_HD inline uint32_t git_header(uint32_t type, uint32_t size, uint32_t hw[kHeaderWords]) {
  MD_SHA_UNROLL
  for (uint32_t i = 0; i < kHeaderWords; i++) hw[i] = 0;
  if (type == kPlain || type > kMaxType) return 0;
  // the digits and the NUL behind them: at most 11 bytes, gathered at the low end, then moved to the top of 12
  unsigned __int128 acc = 0;
  uint32_t nd = 1;
  const uint32_t p10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};
  MD_SHA_UNROLL
  for (int k = 9; k >= 0; k--)
    if (k == 0 || size >= p10[k]) acc = acc << 8 | ('0' + (size / p10[k]) % 10), nd++;
  acc = (acc << 8) << (96 - 8 * nd);
  const uint32_t d[3] = {(uint32_t)(acc >> 64), (uint32_t)(acc >> 32), (uint32_t)acc};
  if (type == 1) {
    hw[0] = 0x636f6d6du, hw[1] = 0x69742000u;  // "commit "
    header_place<7>(d, hw);
    return 7 + nd;
  }
  if (type == 4) {
    hw[0] = 0x74616720u;  // "tag "
    header_place<4>(d, hw);
    return 4 + nd;
  }
  hw[0] = type == 2 ? 0x74726565u : 0x626c6f62u, hw[1] = 0x20000000u;  // "tree ", "blob "
  header_place<5>(d, hw);
  return 5 + nd;
}

// ---- the host's own SHA-1: one serial message ----
struct Sha1 {
  uint32_t h[5];
  uint64_t len;
  uint8_t buf[64];
};

inline void sha1_init(Sha1 *s) {
  init(s->h);
  s->len = 0;
}

inline void sha1_block_bytes(uint32_t h[5], const uint8_t *p) {
  uint32_t w[16];
  for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | (uint32_t)p[4 * i + 3];
  block(h, w);
}

inline void sha1_update(Sha1 *s, const void *data, size_t n) {
  const uint8_t *p = (const uint8_t *)data;
  size_t fill = (size_t)(s->len & 63);
  s->len += n;
  if (fill) {
    const size_t take = n < 64 - fill ? n : 64 - fill;
    memcpy(s->buf + fill, p, take);
    p += take, n -= take, fill += take;
    if (fill < 64) return;
    sha1_block_bytes(s->h, s->buf);
  }
  for (; n >= 64; p += 64, n -= 64) sha1_block_bytes(s->h, p);
  if (n) memcpy(s->buf, p, n);
}

inline void sha1_final(Sha1 *s, uint8_t digest[20]) {
  const uint64_t bits = s->len * 8;
  size_t fill = (size_t)(s->len & 63);
  s->buf[fill++] = 0x80;
  if (fill > 56) {
    memset(s->buf + fill, 0, 64 - fill);
    sha1_block_bytes(s->h, s->buf);
    fill = 0;
  }
  memset(s->buf + fill, 0, 56 - fill);
  for (int i = 0; i < 8; i++) s->buf[56 + i] = (uint8_t)(bits >> (56 - 8 * i));
  sha1_block_bytes(s->h, s->buf);
  for (int i = 0; i < 20; i++) digest[i] = (uint8_t)(s->h[i >> 2] >> (24 - 8 * (i & 3)));
}

// one buffer, one message: the trailers of a pack and of an idx
inline void sha1_of(const void *p, size_t len, uint8_t digest[20]) {
  Sha1 s;
  sha1_init(&s);
  sha1_update(&s, p, len);
  sha1_final(&s, digest);
}

// SHA-1 of a git object (type 1 .. 4), or of the bytes as they are (kPlain): the kernel's CPU twin
inline void sha1_object(uint32_t type, const uint8_t *data, uint32_t size, uint8_t digest[20]) {
  Sha1 s;
  sha1_init(&s);
  uint32_t hw[kHeaderWords];
  const uint32_t hl = git_header(type, size, hw);
  uint8_t hdr[4 * kHeaderWords];
  for (uint32_t i = 0; i < 4 * kHeaderWords; i++) hdr[i] = (uint8_t)(hw[i >> 2] >> (24 - 8 * (i & 3)));
  sha1_update(&s, hdr, hl);
  sha1_update(&s, data, size);
  sha1_final(&s, digest);
}

}  // namespace sha
}  // namespace md
