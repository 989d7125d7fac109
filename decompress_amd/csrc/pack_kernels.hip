// pack_kernels.hip — git packfiles on the device (md_pack_open, md_pack_read; mdeflate.h), for gfx950.  The idx is read
// on the host (pack_index.hpp) and its offsets are sorted there; the zlib streams go through the batch decoder.
//
//   headers_kernel      one thread per object: the type / size varint, an OFS_DELTA's offset (the base by binary search in
//                       the sorted offsets) or a REF_DELTA's name (by binary search in the idx's names)
//   chain_step_kernel   one round of pointer jumping over the base links: jump <- jump[jump], links <- links + links[jump].
//                       Every round reads one pair of arrays and writes another, so no thread waits for another; after
//                       ceil(log2 n) rounds every chain stands at its root, and what does not is on a cycle
//   chain_finish_kernel depth and root, MD_INVALID_PACK for what is on a cycle or hangs off one
//   verdict_kernel      behind the inflate launch: one thread per stream, its final status
//   delta_sizes_kernel  md_pack_open: base size and result size from the front of a delta's payload
//   apply_kernel        the deltas of one level, one wavefront each (below)
//   repeats_kernel      a selected object that was selected before: copied from its first place, one wavefront each
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "copy_bytes.hpp"
#include "internal.hpp"
#include "mdeflate.h"
#include "pack_lookup.hpp"

namespace md {
namespace pk {

constexpr uint32_t kWave = 64;

// LEB128 at a[*p ..), below n: false when it passes n or does not fit 64 bits
__device__ __forceinline__ bool varint(const uint8_t *__restrict__ a, uint64_t n, uint64_t *p, uint64_t *res) {
  uint64_t v = 0, q = *p;
  for (uint32_t shift = 0;; shift += 7) {
    if (q >= n) return false;
    const uint32_t c = a[q++];
    const uint64_t b = c & 0x7f;
    if (shift >= 64 ? b != 0 : (shift > 57 && (b >> (64 - shift)) != 0)) return false;
    if (shift < 64) v |= b << shift;
    if (!(c & 0x80)) break;
  }
  *p = q;
  *res = v;
  return true;
}

__global__ void headers_kernel(Table t, const uint8_t *__restrict__ pack) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.n) return;
  const uint64_t o = t.off[i], e = t.end[i];  // 12 <= o < e <= pack_len - 20 (the host's check)
  uint64_t p = o, size = 0;
  uint32_t type = 0, base = kNoBase;
  int st = MD_OK;
  {
    uint32_t c = pack[p++];
    type = (c >> 4) & 7;
    size = c & 15;
    for (uint32_t shift = 4; (c & 0x80) && st == MD_OK; shift += 7) {
      if (p >= e) {
        st = MD_INVALID_PACK;
        break;
      }
      c = pack[p++];
      const uint64_t b = c & 0x7f;
      if (shift >= 64 ? b != 0 : (shift > 57 && (b >> (64 - shift)) != 0)) st = MD_INVALID_PACK;
      else if (shift < 64) size |= b << shift;
    }
  }
  if (st == MD_OK && (type == 0 || type == 5)) st = MD_INVALID_PACK;
  if (st == MD_OK && type == 6) {  // OFS_DELTA: the distance back to the base
    uint64_t v = 0;
    uint32_t c = 0x80;
    for (bool first = true; c & 0x80; first = false) {
      if (p >= e || (v >> 56) != 0) {
        st = MD_INVALID_PACK;
        break;
      }
      c = pack[p++];
      v = ((first ? 0 : v + 1) << 7) | (c & 0x7f);
    }
    if (st == MD_OK && (v == 0 || v > o)) st = MD_INVALID_PACK;
    if (st == MD_OK) {
      const uint64_t want = o - v;
      uint64_t lo = 0, hi = t.n;
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (t.sorted_off[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      if (lo < t.n && t.sorted_off[lo] == want) base = t.sorted_obj[lo];
      else st = MD_INVALID_PACK;
    }
  } else if (st == MD_OK && type == 7) {  // REF_DELTA: the base's name
    if (e - p < 20) st = MD_INVALID_PACK;
    else {
      const uint8_t *want = pack + p;
      uint64_t at = 0;
      const bool found = find_name(t.names, 0, t.n_names, [&](uint32_t k) { return want[k]; }, &at);
      if (found) base = t.name_obj ? t.name_obj[at] : (uint32_t)at;
      p += 20;
      if (!found) st = MD_PACK_MISSING_BASE;
      else if (base == i) st = MD_INVALID_PACK;  // (a cycle of one)
    }
  }
  const bool link = st == MD_OK && base != kNoBase;
  t.type[i] = (uint8_t)type;
  t.hsize[i] = size;
  t.zoff[i] = p;
  t.base[i] = base;
  t.status[i] = st;
  t.jump[i] = link ? base : (uint32_t)i;
  t.links[i] = link ? 1u : 0u;
}

__global__ void chain_step_kernel(uint64_t n, const uint32_t *__restrict__ jump_in, const uint32_t *__restrict__ links_in,
                                  uint32_t *__restrict__ jump_out, uint32_t *__restrict__ links_out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = jump_in[i];
  jump_out[i] = jump_in[j];
  links_out[i] = links_in[i] + links_in[j];  // (a root has no links; n < 2^31 objects: at most 2^31 links, no wrap)
}

__global__ void chain_finish_kernel(uint64_t n, const uint32_t *__restrict__ jump, const uint32_t *__restrict__ links,
                                    uint32_t *__restrict__ root, uint32_t *__restrict__ depth, int32_t *__restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // A root has no link.  What stands on a cycle after the rounds has followed 2^rounds links, all of them on the way or
  // on the cycle - and may stand on itself again, so jump[r] == r does not tell a root
  const uint32_t r = jump[i];
  const bool cycle = links[r] != 0;
  root[i] = cycle ? (uint32_t)i : r;
  depth[i] = cycle ? 0 : links[i];
  if (cycle && status[i] == MD_OK) status[i] = MD_INVALID_PACK;
}

__global__ void verdict_kernel(uint32_t count, const Stream *__restrict__ s, const uint64_t *__restrict__ out_len,
                               const uint64_t *__restrict__ consumed, const uint32_t *__restrict__ crc, int32_t *__restrict__ status) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  int st = status[j];
  if (st == MD_UNEXPECTED_END_OF_OUTPUT) st = MD_INVALID_SIZE;  // the stream holds more than the header says
  else if (st == MD_OK && (consumed[j] != s[j].in_len || out_len[j] != s[j].hsize)) st = MD_INVALID_SIZE;
  if (st == MD_OK && crc && crc[j] != s[j].crc) st = MD_INVALID_CHECKSUM;
  status[j] = st;
}

__global__ void delta_sizes_kernel(uint32_t count, const Stream *__restrict__ s, const uint8_t *__restrict__ buf,
                                   const uint64_t *__restrict__ pay_off, uint64_t *__restrict__ base_size, uint64_t *__restrict__ result_size,
                                   int32_t *__restrict__ status) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  uint64_t p = 0, b = 0, r = 0;
  if (status[j] == MD_OK) {
    const uint8_t *a = buf + pay_off[j];
    if (!varint(a, s[j].hsize, &p, &b) || !varint(a, s[j].hsize, &p, &r)) status[j] = MD_INVALID_DELTA, b = r = 0;
  }
  base_size[j] = b;
  result_size[j] = r;
}

// The deltas of one level, one wavefront per delta.  A step looks at kWindow bytes of the payload from an instruction
// start p, one byte a lane.  Every lane takes its byte for an opcode and knows how long the instruction would be (a copy:
// 1 + the set bits of its low 7; an insert: 1 + the opcode).  The scalar unit follows the chain of starts from lane 0
// through the window, one v_readlane a link; the lanes on the chain decode their instruction (the operands of a copy
// are read from memory, they may lie beyond the window), a scan over the lengths gives every instruction its place in
// the output, short ones are moved by their own lane, long ones by the whole wavefront 16 bytes a lane
// (copy_bytes_wave).  The next step begins where the chain left the window.
constexpr uint32_t kOwnLane = 16;  // bytes up to which an instruction's lane moves them itself

__global__ __launch_bounds__(kWave) void apply_kernel(uint32_t count, const Delta *__restrict__ rows, uint8_t *buf, int32_t *status) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t d = blockIdx.x; d < count; d += gridDim.x) {
    const Delta row = rows[d];
    if (status[row.self] != MD_OK) continue;  // (uniform: its payload did not decode)
    if (status[row.base_slot] != MD_OK) {
      if (lane == 0) status[row.self] = MD_INVALID_PACK_BASE;
      continue;
    }
    const uint8_t *__restrict__ pay = buf + row.pay_off, *__restrict__ base = buf + row.base_off;
    uint8_t *__restrict__ out = buf + row.out_off;
    const uint64_t n = row.pay_len, bsz = row.base_size, rsz = row.out_size;
    uint64_t p = 0, v0 = 0, v1 = 0, done = 0;
    bool bad = !varint(pay, n, &p, &v0) || !varint(pay, n, &p, &v1) || v0 != bsz || v1 != rsz;
    while (!bad && p < n) {
      const uint64_t q = p + lane;
      const uint32_t op = q < n ? pay[q] : 0;
      const uint32_t ilen = (op & 0x80) ? 1 + __popc(op & 0x7f) : 1 + op;
      uint64_t starts = 0;
      uint32_t cur = 0;
      while (cur < kWindow && p + cur < n) {
        starts |= 1ull << cur;
        cur += (uint32_t)__builtin_amdgcn_readlane((int)ilen, (int)cur);
      }
      const bool mine = (starts >> lane) & 1;
      uint32_t len = 0;
      const uint8_t *src = pay;
      bool wrong = false;
      if (mine) {
        if (op == 0 || ilen > n - q) wrong = true;  // opcode 0; the payload ends inside the instruction
        else if (op & 0x80) {
          const uint8_t *a = pay + q + 1;
          uint32_t off = 0, size = 0;
          if (op & 0x01) off |= (uint32_t)*a++;
          if (op & 0x02) off |= (uint32_t)*a++ << 8;
          if (op & 0x04) off |= (uint32_t)*a++ << 16;
          if (op & 0x08) off |= (uint32_t)*a++ << 24;
          if (op & 0x10) size |= (uint32_t)*a++;
          if (op & 0x20) size |= (uint32_t)*a++ << 8;
          if (op & 0x40) size |= (uint32_t)*a++ << 16;
          if (size == 0) size = 0x10000;
          if (off > bsz || size > bsz - off) wrong = true;  // the copy leaves the base
          src = base + off;
          len = size;
        } else {
          src = pay + q + 1;
          len = op;
        }
      }
      if (wrong) len = 0;
      // the instructions' places: an inclusive scan of the lengths (64 x 2^24 fits 32 bits)
      uint32_t incl = len;
#pragma unroll
      for (uint32_t o = 1; o < kWave; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += up;
      }
      const uint64_t at = done + (incl - len);
      if (mine && !wrong && (at > rsz || len > rsz - at)) wrong = true;  // output beyond the stated size
      if (__ballot(wrong)) {
        bad = true;
        break;
      }
      if (mine && len <= kOwnLane)
        for (uint32_t k = 0; k < len; k++) out[at + k] = src[k];
      for (uint64_t m = __ballot(mine && len > kOwnLane); m; m &= m - 1) {
        const uint32_t l = (uint32_t)__builtin_ctzll(m);
        const uint64_t s_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uintptr_t)src, (int)l);
        const uint64_t s_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uintptr_t)src >> 32), (int)l);
        const uint32_t a_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)at, (int)l);
        const uint32_t a_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(at >> 32), (int)l);
        const uint32_t ln = (uint32_t)__builtin_amdgcn_readlane((int)len, (int)l);
        copy_bytes_wave(out + ((uint64_t)a_hi << 32 | a_lo), (const uint8_t *)(uintptr_t)(s_hi << 32 | s_lo), ln, lane);
      }
      done += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      p += cur;
    }
    if (!bad && done != rsz) bad = true;  // the payload ended with the result size not reached
    if (bad && lane == 0) status[row.self] = MD_INVALID_DELTA;
  }
}

__global__ __launch_bounds__(kWave) void repeats_kernel(uint32_t count, const Repeat *__restrict__ r, uint8_t *buf) {
  for (uint32_t j = blockIdx.x; j < count; j += gridDim.x) copy_bytes_wave(buf + r[j].dst_off, buf + r[j].src_off, r[j].len, threadIdx.x);
}

}  // namespace pk
}  // namespace md

using namespace md::pk;
static inline uint32_t grid_of(uint64_t n, uint32_t threads) { return (uint32_t)((n + threads - 1) / threads); }
constexpr uint32_t kMaxWaveGrid = 1u << 20;  // wavefronts of a launch that strides over its work

extern "C" int md_launch_pk_headers(const md::pk::Table *t, const uint8_t *pack, hipStream_t stream) {
  if (t->n == 0) return 0;
  hipLaunchKernelGGL(headers_kernel, dim3(grid_of(t->n, 256)), dim3(256), 0, stream, *t, pack);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pk_chain_step(uint64_t n, const uint32_t *jump_in, const uint32_t *links_in, uint32_t *jump_out, uint32_t *links_out,
                                       hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(chain_step_kernel, dim3(grid_of(n, 256)), dim3(256), 0, stream, n, jump_in, links_in, jump_out, links_out);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pk_chain_finish(uint64_t n, const uint32_t *jump, const uint32_t *links, uint32_t *root, uint32_t *depth,
                                         int32_t *status, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(chain_finish_kernel, dim3(grid_of(n, 256)), dim3(256), 0, stream, n, jump, links, root, depth, status);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pk_verdict(uint32_t count, const md::pk::Stream *s, const uint64_t *out_len, const uint64_t *consumed,
                                    const uint32_t *crc, int32_t *status, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(verdict_kernel, dim3(grid_of(count, 256)), dim3(256), 0, stream, count, s, out_len, consumed, crc, status);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pk_delta_sizes(uint32_t count, const md::pk::Stream *s, const uint8_t *buf, const uint64_t *pay_off,
                                        uint64_t *base_size, uint64_t *result_size, int32_t *status, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(delta_sizes_kernel, dim3(grid_of(count, 256)), dim3(256), 0, stream, count, s, buf, pay_off, base_size, result_size, status);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pk_apply(uint32_t count, const md::pk::Delta *d, uint8_t *buf, int32_t *status, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(apply_kernel, dim3(count < kMaxWaveGrid ? count : kMaxWaveGrid), dim3(kWave), 0, stream, count, d, buf, status);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pk_repeats(uint32_t count, const md::pk::Repeat *r, uint8_t *buf, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(repeats_kernel, dim3(count < kMaxWaveGrid ? count : kMaxWaveGrid), dim3(kWave), 0, stream, count, r, buf);
  return (int)hipGetLastError();
}
