// sha1_kernels.hip — SHA-1 of many independent messages (md_sha1_batch_*, the names of md_pack_read / md_pack_verify;
// mdeflate.h), for gfx950.  SHA-1 is serial inside a message, so a message is one lane's and a wavefront takes 64.
//
//   sha1_kernel   one lane per message, at most Args::blocks blocks of it a launch: the state (h[5] and the blocks done)
//                 waits in Args::state between the launches.  The host orders the messages longest first when it knows
//                 the lengths, so the lanes of a wavefront are of similar length and the messages of a later launch are
//                 a prefix of the list.
//   names_kernel  one thread per digest: does it equal the 20 bytes expected of it (the idx's name of a pack's object)?
//
// A message is header + content + 0x80 + zeros + the 64-bit bit length; the header ("<type> <size>\0", sha1_host.hpp's
// git_header, at most 18 bytes) is the kernel's own, the content is Args::data[off, off + len).  A block that lies wholly
// in the content is read as aligned dwords and funnelled by the lane's own byte shift (v_alignbyte_b32); block 0 (it holds
// the header) and the last one or two (tail, 0x80, zeros, length) are put together byte by byte.  No dword is read that
// holds no byte of the message, so the buffer may end with the message.  The 80 rounds and the schedule's ring are
// sha1_host.hpp's block(): all of it stays in registers, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "mdeflate.h"
#include "sha1_host.hpp"

namespace md {
namespace sha {

constexpr uint32_t kWave = 64;

__global__ __launch_bounds__(kWave) void sha1_kernel(Args a) {
  const uint32_t lane_msg = blockIdx.x * kWave + threadIdx.x;
  if (lane_msg >= a.count) return;
  const uint32_t m = a.index ? a.index[lane_msg] : lane_msg;
  const uint64_t off = a.off[m], len = a.len[m];
  const uint32_t type = a.type ? a.type[m] : kPlain;
  State *st = a.state + m;
  uint32_t h[5], done = 0;
  if (a.fresh) init(h);
  else {
#pragma unroll
    for (int i = 0; i < 5; i++) h[i] = st->h[i];
    done = st->done;
  }
  uint32_t hw[kHeaderWords];
  const uint32_t hl = git_header(type, (uint32_t)len, hw);
  const uint64_t total = hl + len;                  // bytes in front of the 0x80
  const uint64_t nblocks = (total + 9 + 63) >> 6;   // at most 2^26 + 1
  if (done >= nblocks) return;                      // (finished in an earlier launch: its digest is written)
  const uint64_t end = nblocks - done < a.blocks ? nblocks : (uint64_t)done + a.blocks;
  const uint8_t *__restrict__ content = a.data + off;
  for (uint64_t blk = done; blk < end; blk++) {
    const uint64_t p = blk << 6;  // the block is message[p, p + 64)
    uint32_t w[16];
    if (p >= hl && p + 64 <= total) {
      // wholly content: 16 aligned dwords, and a 17th where the lane's bytes reach into it
      const uintptr_t at = (uintptr_t)(content + (p - hl));
      const uint32_t shift = (uint32_t)(at & 3);
      const uint32_t *__restrict__ q = (const uint32_t *)(at - shift);
      uint32_t x[17];
#pragma unroll
      for (int i = 0; i < 16; i++) x[i] = q[i];
      x[16] = shift ? q[16] : 0;
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = __builtin_bswap32(__builtin_amdgcn_alignbyte(x[i + 1], x[i], shift));
    } else {
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = 0;
      if (blk == 0) {
#pragma unroll
        for (uint32_t i = 0; i < kHeaderWords; i++) w[i] = hw[i];
      }
#pragma unroll
      for (uint32_t k = 0; k < 64; k++) {
        const uint64_t pos = p + k;
        uint32_t byte = 0;
        if (pos >= hl && pos < total) byte = content[pos - hl];
        else if (pos == total) byte = 0x80;
        w[k >> 2] |= byte << (24 - 8 * (k & 3));
      }
      if (blk + 1 == nblocks) {
        const uint64_t bits = total << 3;
        w[14] = (uint32_t)(bits >> 32);
        w[15] = (uint32_t)bits;
      }
    }
    block(h, w);
  }
#pragma unroll
  for (int i = 0; i < 5; i++) st->h[i] = h[i];
  st->done = (uint32_t)end;
  if (end == nblocks) {
    uint8_t *__restrict__ d = a.digest + (uint64_t)m * 20;
#pragma unroll
    for (uint32_t i = 0; i < 20; i++) d[i] = (uint8_t)(h[i >> 2] >> (24 - 8 * (i & 3)));
  }
}

__global__ void names_kernel(uint32_t count, const uint8_t *__restrict__ digest, const uint8_t *__restrict__ expect, uint32_t *__restrict__ differs) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  uint32_t bad = 0;
  for (uint32_t i = 0; i < 20; i++) bad |= (uint32_t)(digest[(uint64_t)j * 20 + i] ^ expect[(uint64_t)j * 20 + i]);
  differs[j] = bad != 0;
}

}  // namespace sha
}  // namespace md

extern "C" int md_launch_sha1(const md::sha::Args *args, hipStream_t stream) {
  if (args->count == 0 || args->blocks == 0) return 0;
  const uint32_t grid = (args->count + md::sha::kWave - 1) / md::sha::kWave;
  hipLaunchKernelGGL(md::sha::sha1_kernel, dim3(grid), dim3(md::sha::kWave), 0, stream, *args);
  return (int)hipGetLastError();
}

extern "C" int md_launch_sha1_names(uint32_t count, const uint8_t *digest, const uint8_t *expect, uint32_t *differs, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(md::sha::names_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, count, digest, expect, differs);
  return (int)hipGetLastError();
}
