// inflate_batch.hip — the hand-out step of many streaming decoders (md_inf_batch_*, stream_inf.cpp), for gfx950.
//
// A round of md_inf_batch_decode is one launch of the inflate kernel over the pieces of every decoder that has new input
// (md_inflate_continue_batch_device: start bit, window and Adler state in, the last block boundary out).  These kernels
// read its results where they lie and leave the host two copies to make, whatever the number of decoders:
//   inf_hand_scan_kernel  one workgroup: the range each row hands out - [hist, resume_out) while its stream goes on,
//                         [hist, out_len) once it ends or fails, nothing when its output room ran out - and an exclusive
//                         scan of the lengths (16-byte aligned) over all rows, in tiles of 1 024; writes struct HandRow.
//   inf_hand_pack_kernel  grid (chunks, rows), rows strided past gridDim.y: packs the handed ranges into one contiguous
//                         blob with 16-byte stores, 64 KiB per workgroup and step; for GZIP each wavefront also takes the
//                         CRC-32 of a quarter of its chunk (crc32_wave) and XORs it, multiplied by x^(8 * bytes after it),
//                         into the row's CRC (crc(A || B) = crc(A) x^(8|B|) xor crc(B): the order of the XORs is free).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gz_crc.hpp"
#include "inflate_batch.hpp"
#include "mdeflate.h"

namespace md {
namespace ib {

constexpr uint32_t kScanThreads = 1024, kScanWaves = kScanThreads / 64;
constexpr uint32_t kPackThreads = 256, kPackChunk = 65536, kPackChunksX = 8;

__global__ __launch_bounds__(kScanThreads) void inf_hand_scan_kernel(uint32_t m, HandIn in, HandRow *__restrict__ res) {
  __shared__ uint64_t wsum[kScanWaves];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < m; base += kScanThreads) {
    const uint32_t r = base + t;
    HandRow h{};
    if (r < m) {
      const int32_t st = in.status[r];
      const uint32_t fl = in.flags[r];
      const uint64_t cap = in.out_cap[r], hist = in.hist[r];
      uint64_t end;
      if (st == MD_UNEXPECTED_END_OF_OUTPUT && (fl & kRowCanGrow)) {
        h.kind = kKindGrow;
        end = hist;
      } else if (st == MD_UNEXPECTED_END_OF_INPUT && !(fl & kRowFinal)) {
        h.kind = kKindContinue;
        end = in.resume_out[r];
        h.tail_bits = in.resume_bits[r];
        h.sum = in.resume_adler[r];
      } else {
        h.kind = kKindFinish;
        end = in.out_len[r];
        h.tail_bits = in.consumed[r] * 8;
        h.sum = in.checksum[r];
      }
      if (end > cap) end = cap;
      if (end < hist) end = hist;  // (a stream the kernel refused wrote nothing)
      h.end = end;
      h.len = end - hist;
      h.status = st;
    }
    // exclusive scan of the padded lengths: inside each wavefront, then over the wavefronts' totals
    const uint64_t pad = (h.len + 15) & ~(uint64_t)15;
    uint64_t x = pad;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint64_t y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    if (w == 0) {
      uint64_t v = lane < kScanWaves ? wsum[lane] : 0;
#pragma unroll
      for (uint32_t o = 1; o < kScanWaves; o <<= 1) {
        const uint64_t y = __shfl_up(v, o);
        if (lane >= o) v += y;
      }
      if (lane < kScanWaves) wsum[lane] = v;
    }
    __syncthreads();
    if (r < m) {
      h.pack_off = carry + (w ? wsum[w - 1] : 0) + x - pad;
      res[r] = h;
    }
    carry += wsum[kScanWaves - 1];
    __syncthreads();  // (wsum is written again by the next tile)
  }
}

__global__ __launch_bounds__(kPackThreads) void inf_hand_pack_kernel(uint32_t m, const uint8_t *__restrict__ out,
                                                                     const uint64_t *__restrict__ out_off,
                                                                     const uint32_t *__restrict__ hist, HandRow *res,
                                                                     uint8_t *__restrict__ pack, int with_crc) {
  __shared__ gz::CrcTab tb;
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (with_crc) gz::crc_tables(&tb, lane);  // (uniform: every wavefront writes the same entries)
  for (uint32_t r = blockIdx.y; r < m; r += gridDim.y) {
    const uint64_t len = res[r].len;
    const uint8_t *src = out + out_off[r] + hist[r];
    uint8_t *dst = pack + res[r].pack_off;  // (16-byte aligned)
    for (uint64_t c0 = (uint64_t)blockIdx.x * kPackChunk; c0 < len; c0 += (uint64_t)gridDim.x * kPackChunk) {
      const uint64_t c1 = c0 + kPackChunk < len ? c0 + kPackChunk : len;
      const uint64_t body = c0 + ((c1 - c0) & ~(uint64_t)15);
      for (uint64_t k = c0 + (uint64_t)threadIdx.x * 16; k < body; k += kPackThreads * 16) {
        uint4 v;
        __builtin_memcpy(&v, src + k, 16);  // (the source is where the window left it: unaligned 16-byte loads)
        *reinterpret_cast<uint4 *>(dst + k) = v;
      }
      for (uint64_t k = body + threadIdx.x; k < c1; k += kPackThreads) dst[k] = src[k];
      if (with_crc) {
        constexpr uint64_t q = kPackChunk / (kPackThreads / 64);
        const uint64_t a = c0 + w * q < c1 ? c0 + w * q : c1, b = a + q < c1 ? a + q : c1;
        if (a < b) {  // (uniform in the wavefront)
          const uint32_t c = gz::crc32_wave(&tb, src + a, b - a, lane);
          if (lane == 0) atomicXor(&res[r].crc, gz::gf_mul(gz::gf_xpow8(len - b), c));
        }
      }
    }
  }
}

}  // namespace ib
}  // namespace md

extern "C" int md_launch_inf_handout(uint32_t m, md::ib::HandIn in, const uint8_t *out, md::ib::HandRow *res, uint8_t *pack,
                                     int with_crc, hipStream_t stream) {
  using namespace md::ib;
  if (m == 0) return 0;
  hipLaunchKernelGGL(inf_hand_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, m, in, res);
  hipLaunchKernelGGL(inf_hand_pack_kernel, dim3(kPackChunksX, m < 65535u ? m : 65535u), dim3(kPackThreads), 0, stream, m, out,
                     in.out_off, in.hist, res, pack, with_crc);
  return (int)hipGetLastError();
}
