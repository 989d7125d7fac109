// gz_crc.hpp — CRC-32 on the device (Checkseum.Crc32, as lib/gz.ml uses it), shared by gz_kernels.hip and
// inflate_batch.hip: a wavefront takes a buffer, every lane runs a 4-table CRC over its own contiguous segment, and the
// 64 partial CRCs are joined with
//     crc(A || B) = crc(A) * x^(8|B|) mod P  xor  crc(B)
// (each lane multiplies by x^(8 * bytes after it), one wave XOR).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace md {
namespace gz {

constexpr int kWave = 64;
constexpr uint32_t kPoly = 0xedb88320u;  // reflected CRC-32 polynomial

// ---- GF(2)[x] / P in the reflected representation (bit 31 = x^0) ----
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 4
  for (int k = 0; k < 32; k++) {
    p ^= b & (0u - ((a >> 31) & 1));
    a <<= 1;
    b = (b >> 1) ^ (kPoly & (0u - (b & 1)));
  }
  return p;
}
// x^(8 * nbytes) mod P
__device__ __forceinline__ uint32_t gf_xpow8(uint64_t nbytes) {
  uint32_t sq = 0x00800000u;  // x^8
  uint32_t r = 0x80000000u;   // x^0
  while (nbytes) {
    if (nbytes & 1) r = gf_mul(r, sq);
    sq = gf_mul(sq, sq);
    nbytes >>= 1;
  }
  return r;
}

struct CrcTab {
  uint32_t t[4][256];
};
__device__ __forceinline__ void crc_tables(CrcTab *tb, uint32_t lane) {
  for (uint32_t i = lane; i < 256; i += kWave) {
    uint32_t c = i;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (kPoly & (0u - (c & 1)));
    tb->t[0][i] = c;
  }
  __syncthreads();
  for (uint32_t i = lane; i < 256; i += kWave) {
    uint32_t c = tb->t[0][i];
    for (int k = 1; k < 4; k++) {
      c = tb->t[0][c & 0xff] ^ (c >> 8);
      tb->t[k][i] = c;
    }
  }
  __syncthreads();
}
__device__ __forceinline__ uint32_t crc_word(const CrcTab *tb, uint32_t c, uint32_t w) {
  c ^= w;
  return tb->t[3][c & 0xff] ^ tb->t[2][(c >> 8) & 0xff] ^ tb->t[1][(c >> 16) & 0xff] ^ tb->t[0][c >> 24];
}
// standard CRC-32 (init and final xor ~0) of buf[0, len), whole wave; result on every lane
static __device__ uint32_t crc32_wave(const CrcTab *tb, const uint8_t *buf, uint64_t len, uint32_t lane) {
  // (segments of whole 64-byte lines: a lane takes a line at a time, four 16-byte loads issued together - with one 16-byte
  // load per step the 64 lines a step touches were back in L2 before their other three quarters were asked for: the
  // 32 wavefronts of a CU hold 128 KiB of such lines against 16 KiB of L1, and the kernel ran at a fifth of HBM's rate)
  const uint64_t seg = ((len + kWave - 1) / kWave + 63) & ~(uint64_t)63;
  uint64_t a = (uint64_t)lane * seg, b = a + seg;
  if (a > len) a = len;
  if (b > len) b = len;
  uint32_t c = 0xffffffffu;
  const uint8_t *q = buf + a, *e = buf + b;
  while (q < e && ((uintptr_t)q & 63) != 0) c = tb->t[0][(c ^ *q++) & 0xff] ^ (c >> 8);
  for (; q + 64 <= e; q += 64) {
    const uint4 v0 = *(const uint4 *)q, v1 = *(const uint4 *)(q + 16), v2 = *(const uint4 *)(q + 32), v3 = *(const uint4 *)(q + 48);
    c = crc_word(tb, c, v0.x);
    c = crc_word(tb, c, v0.y);
    c = crc_word(tb, c, v0.z);
    c = crc_word(tb, c, v0.w);
    c = crc_word(tb, c, v1.x);
    c = crc_word(tb, c, v1.y);
    c = crc_word(tb, c, v1.z);
    c = crc_word(tb, c, v1.w);
    c = crc_word(tb, c, v2.x);
    c = crc_word(tb, c, v2.y);
    c = crc_word(tb, c, v2.z);
    c = crc_word(tb, c, v2.w);
    c = crc_word(tb, c, v3.x);
    c = crc_word(tb, c, v3.y);
    c = crc_word(tb, c, v3.z);
    c = crc_word(tb, c, v3.w);
  }
  for (; q + 16 <= e; q += 16) {
    const uint4 v = *(const uint4 *)q;
    c = crc_word(tb, c, v.x);
    c = crc_word(tb, c, v.y);
    c = crc_word(tb, c, v.z);
    c = crc_word(tb, c, v.w);
  }
  while (q < e) c = tb->t[0][(c ^ *q++) & 0xff] ^ (c >> 8);
  c ^= 0xffffffffu;
  if (a == b) c = 0;  // crc of nothing
  uint32_t term = gf_mul(gf_xpow8(len - b), c);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) term ^= __shfl_xor(term, o);
  return term;
}

}  // namespace gz
}  // namespace md
