// zip_kernels.hip — ZIP archives on the device (md_zip_uncompress, md_zip_compress; mdeflate.h), for gfx950.  The
// directory is read on the host (zip_dir.hpp); what comes here is one row per selected entry (md::zip::Row).
//
//   local_kernel     one thread per entry: the 30-byte local header in front of the directory, its signature, its name
//                    against the directory's; where the body lies; the inflate launch's descriptors and a header status
//   segment_kernel   one wavefront per segment of an entry's output: a stored entry's bytes are copied from the archive
//                    (16-byte stores on the destination's alignment, unaligned 16-byte loads, head and tail bytes one by
//                    one), and every entry's segment gets its CRC-32 (gz_crc.hpp's lane CRC) - of the source for a
//                    stored entry, of the decoder's output for a deflated one.  The writer runs it over its input files
//                    without a destination.  segment -> entry: a table the host built (first[e] = the entry's first
//                    segment, seg_entry[s] = its entry)
//   verdict_kernel   one wavefront per entry joins its segment CRCs, crc(A || B) = crc(A) * x^(8|B|) xor crc(B): every
//                    lane a run of consecutive segments, then as gz_crc.hpp's crc32_wave joins its lanes; then the
//                    entry's final status
//   sizes_kernel     the writer: the same join per file, whether its body is the encoder's or the file itself, the
//                    bytes its local header and body take
//   pack_kernel      the writer: grid (64 KiB chunk, file): local header and body into the file image
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gz_crc.hpp"
#include "internal.hpp"
#include "mdeflate.h"

namespace md {
namespace zip {

using gz::CrcTab;
using gz::kWave;

__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }

// src holds bytes [base, limit) of the archive (limit is at most where the directory begins); names: the directory's
// copies of the selected entries' names
__global__ void local_kernel(uint64_t k, const Row *__restrict__ rows, const uint8_t *__restrict__ src, uint64_t base, uint64_t limit,
                             const uint8_t *__restrict__ names, uint64_t *__restrict__ in_off, uint64_t *__restrict__ in_len,
                             uint64_t *__restrict__ out_cap, uint64_t *__restrict__ body_off, int32_t *__restrict__ hstatus,
                             uint8_t *__restrict__ kind) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const Row r = rows[j];
  int st = MD_OK;
  uint64_t body = 0;
  if (r.header_off < base || r.header_off > limit || limit - r.header_off < 30) st = MD_INVALID_ZIP_HEADER;
  else {
    const uint8_t *h = src + (r.header_off - base);
    const uint64_t n = ld16(h + 26), e = ld16(h + 28), room = limit - r.header_off - 30;
    if (ld32(h) != 0x04034b50u || n != r.name_len || room < n + e || room - n - e < r.csize) st = MD_INVALID_ZIP_HEADER;
    else {
      const uint8_t *a = h + 30, *b = names + r.name_pos;
      uint32_t diff = 0;
      for (uint32_t i = 0; i < n; i++) diff |= (uint32_t)(a[i] ^ b[i]);
      if (diff) st = MD_INVALID_ZIP_HEADER;
      body = r.header_off - base + 30 + n + e;
    }
  }
  if (st == MD_OK) {
    if ((r.flags & (1u | 1u << 6 | 1u << 13)) || (r.method != 0 && r.method != 8)) st = MD_ZIP_UNSUPPORTED;
    else if (r.method == 0 && r.csize != r.usize) st = MD_INVALID_SIZE;
  }
  const bool inflate = st == MD_OK && r.method == 8;
  hstatus[j] = st;
  kind[j] = st != MD_OK ? kSkip : r.method == 0 ? kStored : kDeflated;
  body_off[j] = body;
  in_off[j] = inflate ? body : 0;
  in_len[j] = inflate ? r.csize : 0;
  out_cap[j] = inflate ? r.usize : 0;
}

// n bytes a -> o by one wavefront: 16-byte stores on o's alignment, a read with unaligned 16-byte loads
__device__ __forceinline__ void wave_copy(uint8_t *__restrict__ o, const uint8_t *__restrict__ a, uint64_t n, uint32_t lane) {
  const uint64_t head = (16 - ((uintptr_t)o & 15)) & 15, h1 = head < n ? head : n;
  if (lane < h1) o[lane] = a[lane];
  const uint64_t body = (n - h1) & ~(uint64_t)15;
  for (uint64_t i = h1 + (uint64_t)lane * 16; i < h1 + body; i += kWave * 16) {
    uint4 v;
    __builtin_memcpy(&v, a + i, 16);
    *reinterpret_cast<uint4 *>(o + i) = v;
  }
  const uint64_t t = h1 + body + lane;
  if (t < n) o[t] = a[t];
}

// Segment s of entry e = seg_entry[s] covers bytes [(s - first[e]) * seg, + seg) of the entry's len[e] bytes.  kind[e]:
// kStored: the bytes are src[src_off[e] ..]; they are copied to out[out_off[e] ..] unless out is null; kDeflated: the bytes
// are out[out_off[e] ..]; kSkip: nothing.  crc[s] = the segment's CRC-32.
__global__ __launch_bounds__(kWave) void segment_kernel(uint64_t nseg, uint64_t seg, const uint32_t *__restrict__ seg_entry,
                                                        const uint64_t *__restrict__ first, const uint64_t *__restrict__ len,
                                                        const uint8_t *__restrict__ kind, const uint8_t *__restrict__ src,
                                                        const uint64_t *__restrict__ src_off, uint8_t *out,
                                                        const uint64_t *__restrict__ out_off, uint32_t *__restrict__ crc) {
  __shared__ CrcTab tb;
  const uint32_t lane = threadIdx.x;
  gz::crc_tables(&tb, lane);
  for (uint64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
    const uint32_t e = seg_entry[s];
    const uint64_t at = (s - first[e]) * seg, total = len[e], n = total - at < seg ? total - at : seg;
    const uint32_t what = kind[e];
    uint32_t c = 0;
    if (what == kStored) {  // (uniform)
      const uint8_t *a = src + src_off[e] + at;
      if (out) wave_copy(out + out_off[e] + at, a, n, lane);
      c = gz::crc32_wave(&tb, a, n, lane);
    } else if (what == kDeflated) {
      c = gz::crc32_wave(&tb, out + out_off[e] + at, n, lane);
    }
    if (lane == 0) crc[s] = c;
  }
}

// the CRC-32 of an entry of `total` bytes from its segments' (whole wavefront; the result on every lane)
__device__ __forceinline__ uint32_t join_crc(const uint32_t *__restrict__ crc, uint64_t s0, uint64_t s1, uint64_t seg, uint64_t total,
                                             uint32_t lane) {
  const uint64_t m = s1 - s0, run = (m + kWave - 1) / kWave;
  uint64_t a = lane * run, b = a + run;
  if (a > m) a = m;
  if (b > m) b = m;
  uint32_t c = 0;
  if (a < b) {
    const uint32_t xseg = gz::gf_xpow8(seg);
    for (uint64_t s = a; s < b; s++) {
      const uint64_t n = total - s * seg < seg ? total - s * seg : seg;
      c = gz::gf_mul(c, n == seg ? xseg : gz::gf_xpow8(n)) ^ crc[s0 + s];
    }
  }
  const uint64_t done = b * seg < total ? b * seg : total;
  uint32_t term = gz::gf_mul(gz::gf_xpow8(total - done), c);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) term ^= __shfl_xor(term, o);
  return term;
}

__global__ __launch_bounds__(kWave) void verdict_kernel(uint64_t k, const Row *__restrict__ rows, const uint64_t *__restrict__ first,
                                                        uint64_t seg, const uint32_t *__restrict__ crc, const int32_t *__restrict__ hstatus,
                                                        const uint64_t *__restrict__ out_len, const uint64_t *__restrict__ consumed,
                                                        int32_t *__restrict__ status, unsigned long long *__restrict__ failed) {
  const uint32_t lane = threadIdx.x;
  for (uint64_t j = blockIdx.x; j < k; j += gridDim.x) {
    const uint64_t usize = rows[j].usize, csize = rows[j].csize;
    const bool deflated = rows[j].method == 8;
    int st = hstatus[j];
    if (st == MD_OK && deflated) {
      st = status[j];
      if (st == MD_OK && (consumed[j] != csize || out_len[j] != usize)) st = MD_INVALID_SIZE;
    }
    if (st == MD_OK && join_crc(crc, first[j], first[j + 1], seg, usize, lane) != rows[j].crc) st = MD_INVALID_CHECKSUM;  // (uniform)
    if (lane == 0) {
      status[j] = st;
      if (st != MD_OK) atomicAdd(failed, 1ull);
    }
  }
}

// ---- the writer ----
// the body of file i is the encoder's when it came out shorter than the file
__device__ __forceinline__ bool deflated_body(int level, int st, uint64_t body, uint64_t n) { return level != 0 && st == MD_OK && body < n; }

// rec[4 i ..]: CRC-32, body size, method; (pack_kernel adds the local header's offset)
__global__ __launch_bounds__(kWave) void sizes_kernel(uint64_t n, int level, const uint64_t *__restrict__ in_len, const uint32_t *__restrict__ name_len,
                                                      const uint64_t *__restrict__ out_len, const int32_t *__restrict__ status,
                                                      const uint64_t *__restrict__ first, uint64_t seg, const uint32_t *__restrict__ crc,
                                                      uint64_t *__restrict__ lsize, uint32_t *__restrict__ rec, int32_t *__restrict__ err) {
  const uint32_t lane = threadIdx.x;
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t len = in_len[i];
    const int st = level != 0 ? status[i] : MD_OK;
    const bool d = deflated_body(level, st, level != 0 ? out_len[i] : 0, len);
    const uint32_t c = join_crc(crc, first[i], first[i + 1], seg, len, lane);
    if (lane == 0) {
      // (a body that did not fit its slot of len bytes is not shorter than the file)
      if (st != MD_OK && st != MD_UNEXPECTED_END_OF_OUTPUT) atomicMax(err, st);
      const uint64_t body = d ? out_len[i] : len;
      lsize[i] = 30 + name_len[i] + body;
      rec[4 * i] = c;
      rec[4 * i + 1] = (uint32_t)body;
      rec[4 * i + 2] = d ? 8u : 0u;
    }
  }
}

constexpr uint32_t kPackChunk = 65536;
// n bytes a -> o, 256 threads (as wave_copy)
__device__ __forceinline__ void block_copy(uint8_t *__restrict__ o, const uint8_t *__restrict__ a, uint64_t n) {
  const uint64_t head = (16 - ((uintptr_t)o & 15)) & 15, h1 = head < n ? head : n;
  if (threadIdx.x < h1) o[threadIdx.x] = a[threadIdx.x];
  const uint64_t body = (n - h1) & ~(uint64_t)15;
  for (uint64_t i = h1 + (uint64_t)threadIdx.x * 16; i < h1 + body; i += 256 * 16) {
    uint4 v;
    __builtin_memcpy(&v, a + i, 16);
    *reinterpret_cast<uint4 *>(o + i) = v;
  }
  const uint64_t t = h1 + body + threadIdx.x;
  if (t < n) o[t] = a[t];
}

// loff: n + 1 offsets of the local headers in dst (the scan of lsize).  dos[i] = time | date << 16.
__global__ __launch_bounds__(256) void pack_kernel(uint64_t n, const uint8_t *__restrict__ src, const uint64_t *__restrict__ in_off,
                                                   const uint64_t *__restrict__ in_len, const uint8_t *__restrict__ slots,
                                                   const uint64_t *__restrict__ slot_off, const uint8_t *__restrict__ names,
                                                   const uint64_t *__restrict__ name_pos, const uint32_t *__restrict__ name_len,
                                                   const uint32_t *__restrict__ dos, const uint64_t *__restrict__ loff, uint32_t *__restrict__ rec,
                                                   uint8_t *__restrict__ dst) {
  for (uint64_t i = blockIdx.y; i < n; i += gridDim.y) {
    const uint32_t nl = name_len[i], csize = rec[4 * i + 1], method = rec[4 * i + 2];
    uint8_t *o = dst + loff[i];
    if (blockIdx.x == 0) {
      const uint8_t *nm = names + name_pos[i];
      uint32_t high = 0;  // a byte >= 0x80 in the name: the UTF-8 flag
      for (uint32_t t = threadIdx.x; t < nl; t += 256) {
        const uint8_t b = nm[t];
        o[30 + t] = b;
        high |= b >> 7;
      }
      high = __syncthreads_or((int)high) ? 0x0800u : 0u;
      if (threadIdx.x < 30) {
        const uint32_t t = threadIdx.x, usize = (uint32_t)in_len[i];
        // signature, version needed, flags, method, time, date, CRC-32, csize, usize, name length, extra length
        const uint32_t w = t < 4 ? 0x04034b50u : t < 6 ? (method ? 20u : 10u) : t < 8 ? high : t < 10 ? method : t < 14 ? dos[i]
                           : t < 18 ? rec[4 * i] : t < 22 ? csize : t < 26 ? usize : t < 28 ? nl : 0u;
        const uint32_t at = t < 4 ? 0 : t < 6 ? 4 : t < 8 ? 6 : t < 10 ? 8 : t < 14 ? 10 : t < 18 ? 14 : t < 22 ? 18 : t < 26 ? 22 : t < 28 ? 26 : 28;
        o[t] = (uint8_t)(w >> (8 * (t - at)));
      }
      if (threadIdx.x == 32) rec[4 * i + 3] = (uint32_t)loff[i];
    }
    const uint8_t *a = method ? slots + slot_off[i] : src + in_off[i];
    for (uint64_t c0 = (uint64_t)blockIdx.x * kPackChunk; c0 < csize; c0 += (uint64_t)gridDim.x * kPackChunk)
      block_copy(o + 30 + nl + c0, a + c0, csize - c0 < kPackChunk ? csize - c0 : kPackChunk);
  }
}

}  // namespace zip
}  // namespace md

using namespace md::zip;
static inline uint32_t grid_of(uint64_t n, uint32_t threads) { return (uint32_t)((n + threads - 1) / threads); }
constexpr uint64_t kMaxWaveGrid = 1u << 20;  // wavefronts of a launch that strides over its work

extern "C" int md_launch_zip_local(uint64_t k, const md::zip::Row *rows, const uint8_t *src, uint64_t base, uint64_t limit, const uint8_t *names,
                                   uint64_t *in_off, uint64_t *in_len, uint64_t *out_cap, uint64_t *body_off, int32_t *hstatus, uint8_t *kind,
                                   hipStream_t stream) {
  if (k == 0) return 0;
  hipLaunchKernelGGL(local_kernel, dim3(grid_of(k, 256)), dim3(256), 0, stream, k, rows, src, base, limit, names, in_off, in_len, out_cap,
                     body_off, hstatus, kind);
  return (int)hipGetLastError();
}
extern "C" int md_launch_zip_segments(uint64_t nseg, uint64_t seg, const uint32_t *seg_entry, const uint64_t *first, const uint64_t *len,
                                      const uint8_t *kind, const uint8_t *src, const uint64_t *src_off, uint8_t *out, const uint64_t *out_off,
                                      uint32_t *crc, hipStream_t stream) {
  if (nseg == 0) return 0;
  hipLaunchKernelGGL(segment_kernel, dim3((uint32_t)(nseg < kMaxWaveGrid ? nseg : kMaxWaveGrid)), dim3(kWave), 0, stream, nseg, seg, seg_entry,
                     first, len, kind, src, src_off, out, out_off, crc);
  return (int)hipGetLastError();
}
extern "C" int md_launch_zip_verdict(uint64_t k, const md::zip::Row *rows, const uint64_t *first, uint64_t seg, const uint32_t *crc,
                                     const int32_t *hstatus, const uint64_t *out_len, const uint64_t *consumed, int32_t *status, uint64_t *failed,
                                     hipStream_t stream) {
  if (k == 0) return 0;
  hipLaunchKernelGGL(verdict_kernel, dim3((uint32_t)(k < kMaxWaveGrid ? k : kMaxWaveGrid)), dim3(kWave), 0, stream, k, rows, first, seg, crc,
                     hstatus, out_len, consumed, status, (unsigned long long *)failed);
  return (int)hipGetLastError();
}
extern "C" int md_launch_zip_sizes(uint64_t n, int level, const uint64_t *in_len, const uint32_t *name_len, const uint64_t *out_len,
                                   const int32_t *status, const uint64_t *first, uint64_t seg, const uint32_t *crc, uint64_t *lsize, uint32_t *rec,
                                   int32_t *err, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(sizes_kernel, dim3((uint32_t)(n < kMaxWaveGrid ? n : kMaxWaveGrid)), dim3(kWave), 0, stream, n, level, in_len, name_len,
                     out_len, status, first, seg, crc, lsize, rec, err);
  return (int)hipGetLastError();
}
extern "C" int md_launch_zip_pack(uint64_t n, uint64_t longest, const uint8_t *src, const uint64_t *in_off, const uint64_t *in_len,
                                  const uint8_t *slots, const uint64_t *slot_off, const uint8_t *names, const uint64_t *name_pos,
                                  const uint32_t *name_len, const uint32_t *dos, const uint64_t *loff, uint32_t *rec, uint8_t *dst,
                                  hipStream_t stream) {
  if (n == 0) return 0;
  // chunks of the longest file, at most 64 workgroups a file: the rest strides
  const uint64_t chunks = (longest + kPackChunk - 1) / kPackChunk;
  const uint32_t gx = (uint32_t)(chunks < 1 ? 1 : chunks > 64 ? 64 : chunks);
  hipLaunchKernelGGL(pack_kernel, dim3(gx, (uint32_t)(n < 65535 ? n : 65535)), dim3(256), 0, stream, n, src, in_off, in_len, slots, slot_off,
                     names, name_pos, name_len, dos, loff, rec, dst);
  return (int)hipGetLastError();
}
