// pack_delta_walk.hpp — what the kernels that make deltas (pack_write_kernels.hip) and the ones that choose bases
// (pack_search_kernels.hip) share on the device: the unaligned 16-byte block, its hash, and the walk of one wavefront over
// one (base, target) pair.  delta_walk<true> writes the delta of mdeflate.h's definition; delta_walk<false> takes the same
// steps and only counts, so a length it reports is the length the writer would have reached, op for op.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "copy_bytes.hpp"
#include "internal.hpp"
#include "mdeflate.h"

namespace md {
namespace pkw {

constexpr uint32_t kWave = 64;

struct Block {
  uint32_t w[4];
};

// 16 bytes at any address
__device__ __forceinline__ Block load_block(const uint8_t *__restrict__ a) {
  Block b;
  __builtin_memcpy(&b, a, 16);
  return b;
}

__device__ __forceinline__ uint32_t hash_block(const Block &b) {
  uint32_t x = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) x = (x + b.w[i]) * kHashMul;
  return x;
}

__device__ __forceinline__ bool same_block(const Block &a, const Block &b) {
  return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3])) == 0;
}

// bytes of [0, n) (n <= 16) in which a and b agree from the front / from the back.  a and b point at the 16 bytes' first;
// fewer than 16 are read one by one, so no byte outside [0, n) is touched.
__device__ __forceinline__ uint32_t equal_front(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t n) {
  if (n == kBlock) {
    const Block x = load_block(a), y = load_block(b);
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
      const uint32_t d = x.w[i] ^ y.w[i];
      if (d) return 4 * i + ((uint32_t)__builtin_ctz(d) >> 3);
    }
    return kBlock;
  }
  uint32_t k = 0;
  while (k < n && a[k] == b[k]) k++;
  return k;
}
// here a and b point BEHIND the last byte: the bytes are a[-n .. -1]
__device__ __forceinline__ uint32_t equal_back(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t n) {
  if (n == kBlock) {
    const Block x = load_block(a - kBlock), y = load_block(b - kBlock);
#pragma unroll
    for (int i = 3; i >= 0; i--) {
      const uint32_t d = x.w[i] ^ y.w[i];
      if (d) return 4 * (3 - (uint32_t)i) + ((uint32_t)__builtin_clz(d) >> 3);
    }
    return kBlock;
  }
  uint32_t k = 0;
  while (k < n && a[-(int)k - 1] == b[-(int)k - 1]) k++;
  return k;
}

__device__ __forceinline__ uint32_t uniform(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }

// a varint by lane 0; returns its length
__device__ __forceinline__ uint32_t put_varint(uint8_t *__restrict__ o, uint64_t v, bool write) {
  uint32_t k = 0;
  for (;; k++) {
    const uint32_t c = (uint32_t)(v & 0x7f);
    v >>= 7;
    if (write) o[k] = (uint8_t)(c | (v ? 0x80 : 0));
    if (!v) return k + 1;
  }
}
__device__ __forceinline__ uint32_t varint_len(uint64_t v) {
  uint32_t k = 1;
  while (v >>= 7) k++;
  return k;
}

// One wavefront on one pair.  Everything that steers the loop - lit, the scan position, the output position, a match's p, j,
// L, e - is the same in all lanes (ballots and v_readlane), so no lane waits for another.
//  scan     64 target positions a step from `lit`: lane l hashes the 16 bytes at its position, reads its slot and, where the
//           slot holds a block, compares the block with its 16 bytes; a ballot's lowest bit is the first hit
//  forward  1 024 bytes a step, 16 a lane, behind the block; a lane stops where its bytes differ or either buffer ends; the
//           ballot's lowest stopped lane ends the run with the bytes it found equal
//  backward the same towards lit and the base's start
//  emit     the literals T[lit, p - e) as inserts of at most 127 bytes - lane 0 writes the count, all lanes move the bytes -
//           and the copy in ops of at most 0x10000 bytes, lane 0 alone
// The output position is checked against out_cap before every op: the first op that would pass it ends the pair with
// *full set (what was written stays below out_cap).  kWrite false: `out` is never touched, the position moves as it would.
// Returns the output position.
template <bool kWrite>
__device__ __forceinline__ uint64_t delta_walk(const Pair &row, const uint8_t *__restrict__ src, const uint32_t *__restrict__ tables,
                                               uint8_t *__restrict__ out, uint32_t lane, bool *is_full) {
  const uint8_t *__restrict__ B = src + row.base_off, *__restrict__ T = src + row.tgt_off;
  const uint32_t *__restrict__ table = tables + row.table_off;
  const uint32_t nb = (uint32_t)row.base_len, nt = (uint32_t)row.tgt_len;  // (at most MD_MAX_STREAM: 32 bits)
  const uint64_t cap = row.out_cap;
  const uint32_t shift = 32 - row.bits;
  uint64_t o = 0;
  bool full = false;

  // inserts of T[from, to)
  auto literals = [&](uint32_t from, uint32_t to) {
    while (from < to && !full) {
      const uint32_t n = to - from < kMaxInsert ? to - from : kMaxInsert;
      if (o + 1 + n > cap) {
        full = true;
        break;
      }
      if constexpr (kWrite) {
        if (lane == 0) out[o] = (uint8_t)n;
        copy_bytes_wave(out + o + 1, T + from, n, lane);
      }
      o += 1 + n;
      from += n;
    }
  };
  // copies of B[off, off + size)
  auto copies = [&](uint32_t off, uint32_t size) {
    while (size && !full) {
      const uint32_t n = size < kMaxCopy ? size : kMaxCopy, sz = n == kMaxCopy ? 0 : n;
      const uint32_t len = 1 + ((off & 0xff) != 0) + ((off & 0xff00) != 0) + ((off & 0xff0000) != 0) + ((off >> 24) != 0) + ((sz & 0xff) != 0) +
                           ((sz & 0xff00) != 0);
      if (o + len > cap) {
        full = true;
        break;
      }
      if constexpr (kWrite) {
        if (lane == 0) {
          uint8_t *q = out + o + 1;
          uint32_t cmd = 0x80;
#pragma unroll
          for (uint32_t i = 0; i < 4; i++)
            if ((off >> (8 * i)) & 0xff) cmd |= 1u << i, *q++ = (uint8_t)(off >> (8 * i));
#pragma unroll
          for (uint32_t i = 0; i < 2; i++)
            if ((sz >> (8 * i)) & 0xff) cmd |= 0x10u << i, *q++ = (uint8_t)(sz >> (8 * i));
          out[o] = (uint8_t)cmd;
        }
      }
      o += len;
      off += n;
      size -= n;
    }
  };

  {  // varint(nb) varint(nt)
    const uint32_t head = varint_len(nb) + varint_len(nt);
    if (head > cap) full = true;
    else {
      if constexpr (kWrite) {
        const uint32_t k = put_varint(out, nb, lane == 0);
        put_varint(out + k, nt, lane == 0);
      }
      o = head;
    }
  }
  uint32_t lit = 0, scan = 0;
  const uint32_t nblocks = nb / kBlock;
  while (!full && nblocks && nt >= kBlock && scan <= nt - kBlock) {
    const uint64_t q = (uint64_t)scan + lane;
    uint32_t j = kEmpty;
    bool hit = false;
    if (q <= nt - kBlock) {
      const Block t = load_block(T + q);
      j = table[hash_block(t) >> shift];
      if (j != kEmpty) hit = same_block(t, load_block(B + (uint64_t)j * kBlock));  // (j < nblocks: the index kernel's)
    }
    const uint64_t m = __ballot(hit);
    if (m == 0) {
      if (nt - scan <= kWave) break;  // (no wrap near 2^32)
      scan += kWave;
      continue;
    }
    const uint32_t first = (uint32_t)__builtin_ctzll(m);
    const uint32_t p = scan + first;
    j = uniform(j, first);
    // forward, behind the block
    const uint32_t bf = j * kBlock + kBlock, tf = p + kBlock;
    const uint32_t maxf = nb - bf < nt - tf ? nb - bf : nt - tf;
    uint32_t L = 0;
    for (;;) {
      const uint32_t rem = maxf - L, lo = lane * kBlock;
      const uint32_t n = lo >= rem ? 0 : (rem - lo < kBlock ? rem - lo : kBlock);
      const uint64_t c = (uint64_t)L + lo;
      const uint32_t eq = n ? equal_front(B + bf + c, T + tf + c, n) : 0;
      const uint64_t stop = __ballot(eq < kBlock);
      if (stop == 0) {
        L += kWave * kBlock;
        continue;
      }
      const uint32_t l = (uint32_t)__builtin_ctzll(stop);
      L += l * kBlock + uniform(eq, l);
      break;
    }
    // backward, towards lit and the base's start
    const uint32_t bb = j * kBlock;
    const uint32_t maxb = p - lit < bb ? p - lit : bb;
    uint32_t e = 0;
    for (;;) {
      const uint32_t rem = maxb - e, lo = lane * kBlock;
      const uint32_t n = lo >= rem ? 0 : (rem - lo < kBlock ? rem - lo : kBlock);
      const uint64_t c = (uint64_t)e + lo;
      const uint32_t eq = n ? equal_back(B + bb - c, T + p - c, n) : 0;
      const uint64_t stop = __ballot(eq < kBlock);
      if (stop == 0) {
        e += kWave * kBlock;
        continue;
      }
      const uint32_t l = (uint32_t)__builtin_ctzll(stop);
      e += l * kBlock + uniform(eq, l);
      break;
    }
    literals(lit, p - e);
    copies(bb - e, kBlock + L + e);
    lit = tf + L;
    scan = lit;
  }
  literals(lit, nt);
  *is_full = full;
  return o;
}

}  // namespace pkw
}  // namespace md
