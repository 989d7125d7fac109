// gz_members.hip — a GZip FILE of many members (RFC 1952 2.2) on gfx950: the kernels behind md_gz_members_* and
// md_bgzf_compress (capi.cpp).  RFC semantics (gz_rfc.hpp), not Gz.Inf's.
//
// Reader, for files whose members carry their own size (the `BC` extra subfield of BGZF: bgzip, htslib, .bam):
//   mark_kernel      the whole chip looks at every byte position for the start of an INDEXED member - 1f 8b 08, FLG with
//                    FEXTRA and no reserved bit, and in the extra field a subfield 'B' 'C' of length 2 whose BSIZE + 1
//                    is a member length that fits the header and ends inside the buffer.  16 bytes a thread and step plus
//                    a 4-byte halo; a hit sets one bit of a bitmap (1 bit per input byte); each workgroup leaves its
//                    count, and the chip the end of the last byte that is not NUL.
//   scan_kernel      exclusive prefix sums (one workgroup; the arrays are one entry per 16 KiB of input, per candidate or
//                    per member)
//   compact_kernel   the candidates in position order: position and where the member says the next one starts
//   link_kernel      candidate -> index of the candidate at its end (binary search), or END (the member ends at the end
//                    of the buffer or at NUL bytes that reach it), or DEAD
//   jump_kernel      pointer jumping: after round k every candidate fewer than 2^(k+1) hops from offset 0 is marked, so
//                    ceil(log2) rounds settle which candidates are the file's members and whether the chain reaches END
//   select_kernel    the marked candidates, in order: the members
//   header_kernel    per member: the RFC header, body offset / length, ISIZE from the trailer - in the layout
//                    gz_header_kernel leaves, so the inflate launch (MD_FORMAT_DEFLATE over the bodies, out_cap = ISIZE) and
//                    gz_finish_kernel take the arrays as they are
//   verdict_kernel   a member that overran its ISIZE is MD_INVALID_SIZE; the first member that failed (one atomic min)
// Writer (blocked gzip, every member with a BC field, as bgzip writes):
//   bgzf_plan_kernel   block i of the input -> stream i of the deflate launch, slots of fixed stride
//   bgzf_size_kernel   member sizes: 26 + body, or the stored form (26 + 5 + bytes) where that is the shorter one
//   bgzf_pack_kernel   one workgroup per member writes header, body (or 01 LEN NLEN + the block), CRC-32 and ISIZE at
//                      the member's final offset, 16-byte stores on the destination's alignment; the last workgroup the
//                      28-byte EOF marker
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "copy_bytes.hpp"
#include "gz_rfc.hpp"
#include "internal.hpp"
#include "mdeflate.h"

namespace md {
namespace gzm {

constexpr uint32_t kMarkThreads = 256;
constexpr uint32_t kMarkSteps = 4;
constexpr uint32_t kMarkSpan = kMarkThreads * kMarkSteps * 16;  // input bytes per workgroup
static_assert(kMarkSpan == kMarkSpanBytes, "capi.cpp sizes the counts by this");

__device__ __forceinline__ uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// length of the indexed member that starts at p (p < len), 0 if none does
__device__ uint32_t indexed_member_at(const uint8_t *__restrict__ s, uint64_t len, uint64_t p) {
  if (len - p < 12 + 6 + 2 + 8) return 0;
  const uint8_t *h = s + p;
  if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0xe4) != 4) return 0;
  const uint32_t xlen = le16(h + 10);
  if (len - p - 12 < xlen) return 0;
  for (uint32_t q = 0; q + 4 <= xlen;) {
    const uint8_t *f = h + 12 + q;
    const uint32_t sl = le16(f + 2);
    if (q + 4 + sl > xlen) return 0;
    if (f[0] == 'B' && f[1] == 'C' && sl == 2) {
      const uint32_t m = le16(f + 4) + 1;
      return m < 12 + xlen + 2 + 8 || m > len - p ? 0 : m;
    }
    q += 4 + sl;
  }
  return 0;
}

__global__ __launch_bounds__(kMarkThreads) void mark_kernel(const uint8_t *__restrict__ s, uint64_t len, uint32_t *__restrict__ bits,
                                                            uint32_t *__restrict__ cnt, unsigned long long *__restrict__ last_nz) {
  __shared__ uint32_t found;
  __shared__ unsigned long long nz;
  if (threadIdx.x == 0) {
    found = 0;
    nz = 0;
  }
  __syncthreads();
  unsigned long long my_nz = 0;
  for (uint32_t step = 0; step < kMarkSteps; step++) {
    const uint64_t c = (uint64_t)blockIdx.x * kMarkSpan + ((uint64_t)step * kMarkThreads + threadIdx.x) * 16;
    if (c >= len) break;
    uint32_t w[5] = {0, 0, 0, 0, 0};  // bytes c .. c + 19, NUL behind the end
    if (len - c >= 20) {
      __builtin_memcpy(w, s + c, 16);
      __builtin_memcpy(w + 4, s + c + 16, 4);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 20; k++)  // (unrolled: w[] stays in registers)
        if (c + k < len) w[k >> 2] |= (uint32_t)s[c + k] << (8 * (k & 3));
    }
    bool has1f = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (w[k]) my_nz = c + 4 * k + (31 - __builtin_clz(w[k])) / 8 + 1;
      const uint32_t x = w[k] ^ 0x1f1f1f1fu;
      has1f |= ((x - 0x01010101u) & ~x & 0x80808080u) != 0;
    }
    if (!has1f) continue;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
      if (c + k >= len) break;
      const uint64_t two = ((uint64_t)w[(k >> 2) + 1] << 32) | w[k >> 2];
      const uint32_t sig = (uint32_t)(two >> (8 * (k & 3)));
      if ((sig & 0xe4ffffffu) != 0x04088b1fu) continue;
      const uint64_t p = c + k;
      if (indexed_member_at(s, len, p) == 0) continue;
      atomicOr(&bits[p >> 5], 1u << (p & 31));
      atomicAdd(&found, 1u);
    }
  }
  if (my_nz) atomicMax(&nz, my_nz);
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = found;
    if (nz) atomicMax(last_nz, nz);
  }
}

// out[i] = in[0] + ... + in[i - 1], out[n] = the total; one workgroup of 1 024
__device__ __forceinline__ unsigned long long wave_incl(unsigned long long x, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(x, o);
    if ((int)lane >= o) x += y;
  }
  return x;
}
template <class T>
__global__ __launch_bounds__(1024) void scan_kernel(const T *__restrict__ in, uint64_t n, uint64_t *__restrict__ out) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long carry;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint64_t base = 0; base < n; base += 1024) {
    const uint64_t i = base + threadIdx.x;
    const unsigned long long v = i < n ? (unsigned long long)in[i] : 0;
    const unsigned long long x = wave_incl(v, lane);
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    unsigned long long before = carry;
    for (uint32_t k = 0; k < wave; k++) before += wsum[k];
    if (i < n) out[i] = before + x - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = before + x;
    __syncthreads();
  }
  if (threadIdx.x == 0) out[n] = carry;
}

// workgroup b: the bits mark_kernel's workgroup b set (kMarkSpan / 32 words, two a thread), in position order from base[b]
__global__ __launch_bounds__(kMarkThreads) void compact_kernel(const uint8_t *__restrict__ s, uint64_t len, const uint32_t *__restrict__ bits,
                                                               const uint64_t *__restrict__ base, uint64_t *__restrict__ cpos,
                                                               uint64_t *__restrict__ cnext) {
  __shared__ uint32_t wsum[kMarkThreads / 64];
  const uint64_t b0 = base[blockIdx.x];
  if (base[blockIdx.x + 1] == b0) return;  // (uniform: most spans hold no candidate)
  const uint64_t nwords = (len + 31) / 32;
  const uint64_t w0 = (uint64_t)blockIdx.x * (kMarkSpan / 32) + threadIdx.x * 2;
  uint32_t a[2] = {w0 < nwords ? bits[w0] : 0u, w0 + 1 < nwords ? bits[w0 + 1] : 0u};
  const uint32_t mine = __popc(a[0]) + __popc(a[1]);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t incl = (uint32_t)wave_incl(mine, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint64_t k = b0 + incl - mine;
  for (uint32_t j = 0; j < wave; j++) k += wsum[j];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    while (a[h]) {
      const uint32_t bit = __builtin_ctz(a[h]);
      a[h] &= a[h] - 1;
      const uint64_t p = (w0 + h) * 32 + bit;
      cpos[k] = p;
      cnext[k] = p + indexed_member_at(s, len, p);
      k++;
    }
  }
}

// jump[i]: index of the candidate at cnext[i]; C = END, C + 1 = DEAD (both point at themselves).  reach[] = {offset 0 is a
// candidate} on candidate 0, else 0.
__global__ void link_kernel(uint64_t C, const uint64_t *__restrict__ cpos, const uint64_t *__restrict__ cnext,
                            const unsigned long long *__restrict__ last_nz, uint32_t *__restrict__ jump, uint32_t *__restrict__ reach) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C + 2) return;
  reach[i] = i == 0 && cpos[0] == 0 ? 1u : 0u;
  if (i >= C) {
    jump[i] = (uint32_t)i;
    return;
  }
  const uint64_t t = cnext[i];
  uint64_t lo = i + 1, hi = C;  // (positions ascend, and a member is longer than nothing)
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (cpos[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  jump[i] = lo < C && cpos[lo] == t ? (uint32_t)lo : t >= *last_nz ? (uint32_t)C : (uint32_t)(C + 1);
}

// (a candidate marked in this very round may pass the mark on as well: it lies on the chain from 0 either way)
__global__ void jump_kernel(uint64_t C, const uint32_t *__restrict__ jin, uint32_t *__restrict__ jout, uint32_t *reach) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C + 2) return;
  const uint32_t a = jin[i];
  if (reach[i] && !reach[a]) reach[a] = 1u;
  jout[i] = jin[a];
}

__global__ void select_kernel(uint64_t C, const uint32_t *__restrict__ reach, const uint64_t *__restrict__ ridx,
                              const uint64_t *__restrict__ cpos, const uint64_t *__restrict__ cnext, uint64_t *__restrict__ mpos,
                              uint64_t *__restrict__ mlen) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C || !reach[i]) return;
  mpos[ridx[i]] = cpos[i];
  mlen[ridx[i]] = cnext[i] - cpos[i];
}

__global__ void header_kernel(uint64_t M, const uint8_t *__restrict__ s, const uint64_t *__restrict__ mpos, const uint64_t *__restrict__ mlen,
                              uint64_t *__restrict__ body_off, uint64_t *__restrict__ body_len, uint64_t *__restrict__ isize,
                              int32_t *__restrict__ hstatus) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const uint8_t *m = s + mpos[i];
  const uint64_t len = mlen[i];
  uint64_t hdr = 0;
  int st = gz::rfc_header(m, len, &hdr);
  if (st == MD_OK && len - hdr < 8) st = MD_UNEXPECTED_END_OF_INPUT;
  uint32_t sz = 0;
  if (st == MD_OK)
    for (int k = 0; k < 4; k++) sz |= (uint32_t)m[len - 4 + k] << (8 * k);
  hstatus[i] = st;
  body_off[i] = mpos[i] + (st == MD_OK ? hdr : 0);
  body_len[i] = st == MD_OK ? len - hdr - 8 : 0;
  isize[i] = sz;
}

__global__ void verdict_kernel(uint64_t M, const uint64_t *__restrict__ mlen, const uint64_t *__restrict__ consumed,
                               int32_t *__restrict__ status, unsigned long long *__restrict__ first) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  int st = status[i];
  if (st == MD_UNEXPECTED_END_OF_OUTPUT) st = MD_INVALID_SIZE;  // (out_cap is the member's own ISIZE)
  // the body ended in front of where the size field puts the trailer: what follows is not the member the chain assumed
  if (st == MD_OK && consumed[i] != mlen[i]) st = MD_INVALID_GZIP_HEADER;
  status[i] = st;
  if (st != MD_OK) atomicMin(first, (unsigned long long)i);
}

// ---- the writer ----
__global__ void bgzf_plan_kernel(uint64_t nb, uint64_t len, uint64_t block, uint64_t stride, uint64_t *__restrict__ in_off,
                                 uint64_t *__restrict__ in_len, uint64_t *__restrict__ out_off, uint64_t *__restrict__ out_cap) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  in_off[i] = i * block;
  in_len[i] = len - i * block < block ? len - i * block : block;
  out_off[i] = i * stride;
  out_cap[i] = stride;
}

// 1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 'B' 'C' 2 0 | BSIZE
__constant__ uint8_t fixed[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
constexpr uint32_t kBgzfHeader = 18, kBgzfFrame = 26;
// The encoder's body is kept unless one stored block (5 + n bytes) is shorter: input that does not compress.  With n <=
// 0xff00 no member is then longer than 26 + 5 + 0xff00 = 65 311 <= 65 536, and md_bgzf_compress_bound holds.
__device__ __forceinline__ bool bgzf_deflated(int st, uint64_t body, uint64_t n) { return st == MD_OK && body <= 5 + n; }

__global__ void bgzf_size_kernel(uint64_t nb, const uint64_t *__restrict__ in_len, const uint64_t *__restrict__ out_len,
                                 const int32_t *__restrict__ status, uint64_t *__restrict__ msize, int32_t *__restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const int st = status[i];
  // (a body that did not fit its slot of n + 5 bytes is longer than the stored form)
  if (st != MD_OK && st != MD_UNEXPECTED_END_OF_OUTPUT) atomicMax(err, st);
  msize[i] = bgzf_deflated(st, out_len[i], in_len[i]) ? kBgzfFrame + out_len[i] : kBgzfFrame + 5 + in_len[i];
}

__global__ __launch_bounds__(256) void bgzf_pack_kernel(uint64_t nb, const uint8_t *__restrict__ src, const uint64_t *__restrict__ in_off,
                                                        const uint64_t *__restrict__ in_len, const uint8_t *__restrict__ slots,
                                                        const uint64_t *__restrict__ slot_off, const uint64_t *__restrict__ out_len,
                                                        const int32_t *__restrict__ status, const uint64_t *__restrict__ moff,
                                                        const uint32_t *__restrict__ crc, uint8_t *__restrict__ dst) {
  const uint64_t i = blockIdx.x;
  uint8_t *o = dst + moff[i];
  if (i == nb) {  // the EOF marker: an empty member, body 03 00
    if (threadIdx.x < 16) o[threadIdx.x] = fixed[threadIdx.x];
    else if (threadIdx.x < 28) o[threadIdx.x] = threadIdx.x == 16 ? 0x1b : threadIdx.x == 18 ? 0x03 : 0;
    return;
  }
  const uint64_t n = in_len[i], size = moff[i + 1] - moff[i];
  const bool deflated = bgzf_deflated(status[i], out_len[i], n);
  if (threadIdx.x < 16) o[threadIdx.x] = fixed[threadIdx.x];
  else if (threadIdx.x < 18) o[threadIdx.x] = (uint8_t)((size - 1) >> (8 * (threadIdx.x - 16)));
  else if (threadIdx.x >= 32 && threadIdx.x < 40) {
    const uint32_t k = threadIdx.x - 32;
    o[size - 8 + k] = (uint8_t)((k < 4 ? crc[i] : (uint32_t)n) >> (8 * (k & 3)));
  } else if (!deflated && threadIdx.x >= 64 && threadIdx.x < 69) {  // one stored block, the last: 01 LEN NLEN
    const uint32_t k = threadIdx.x - 64, ln = (uint32_t)n;
    o[kBgzfHeader + k] = k == 0 ? 1 : (uint8_t)((k < 3 ? ln : ~ln) >> (8 * ((k - 1) & 1)));
  }
  if (deflated) copy_bytes(o + kBgzfHeader, slots + slot_off[i], out_len[i]);
  else copy_bytes(o + kBgzfHeader + 5, src + in_off[i], n);
}

}  // namespace gzm
}  // namespace md

using namespace md::gzm;
static inline uint32_t grid_of(uint64_t n, uint32_t threads) { return (uint32_t)((n + threads - 1) / threads); }

extern "C" int md_launch_gzm_mark(const uint8_t *src, uint64_t len, uint32_t *bits, uint32_t *cnt, uint64_t *last_nz, hipStream_t stream) {
  if (len == 0) return 0;
  hipError_t e = hipMemsetAsync(bits, 0, (len + 31) / 32 * 4, stream);
  if (e == hipSuccess) e = hipMemsetAsync(last_nz, 0, 8, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(mark_kernel, dim3(grid_of(len, kMarkSpan)), dim3(kMarkThreads), 0, stream, src, len, bits, cnt, (unsigned long long *)last_nz);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzm_scan32(const uint32_t *in, uint64_t n, uint64_t *out, hipStream_t stream) {
  hipLaunchKernelGGL(scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, stream, in, n, out);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzm_scan64(const uint64_t *in, uint64_t n, uint64_t *out, hipStream_t stream) {
  hipLaunchKernelGGL(scan_kernel<uint64_t>, dim3(1), dim3(1024), 0, stream, in, n, out);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzm_compact(const uint8_t *src, uint64_t len, const uint32_t *bits, const uint64_t *base, uint64_t *cpos,
                                     uint64_t *cnext, hipStream_t stream) {
  if (len == 0) return 0;
  hipLaunchKernelGGL(compact_kernel, dim3(grid_of(len, kMarkSpan)), dim3(kMarkThreads), 0, stream, src, len, bits, base, cpos, cnext);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzm_chain(uint64_t C, const uint64_t *cpos, const uint64_t *cnext, const uint64_t *last_nz, uint32_t *jump_a,
                                   uint32_t *jump_b, uint32_t *reach, hipStream_t stream) {
  const uint32_t g = grid_of(C + 2, 256);
  hipLaunchKernelGGL(link_kernel, dim3(g), dim3(256), 0, stream, C, cpos, cnext, (const unsigned long long *)last_nz, jump_a, reach);
  // END is at most C hops from candidate 0: rounds until 2^rounds > C
  for (uint64_t reachable = 1; reachable <= C; reachable *= 2) {
    hipLaunchKernelGGL(jump_kernel, dim3(g), dim3(256), 0, stream, C, jump_a, jump_b, reach);
    uint32_t *t = jump_a;
    jump_a = jump_b;
    jump_b = t;
  }
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzm_select(uint64_t C, const uint32_t *reach, const uint64_t *ridx, const uint64_t *cpos, const uint64_t *cnext,
                                    uint64_t *mpos, uint64_t *mlen, hipStream_t stream) {
  if (C == 0) return 0;
  hipLaunchKernelGGL(select_kernel, dim3(grid_of(C, 256)), dim3(256), 0, stream, C, reach, ridx, cpos, cnext, mpos, mlen);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzm_headers(uint64_t M, const uint8_t *src, const uint64_t *mpos, const uint64_t *mlen, uint64_t *body_off,
                                     uint64_t *body_len, uint64_t *isize, int32_t *hstatus, hipStream_t stream) {
  if (M == 0) return 0;
  hipLaunchKernelGGL(header_kernel, dim3(grid_of(M, 256)), dim3(256), 0, stream, M, src, mpos, mlen, body_off, body_len, isize, hstatus);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzm_verdict(uint64_t M, const uint64_t *mlen, const uint64_t *consumed, int32_t *status, uint64_t *first,
                                     hipStream_t stream) {
  if (M == 0) return 0;
  hipLaunchKernelGGL(verdict_kernel, dim3(grid_of(M, 256)), dim3(256), 0, stream, M, mlen, consumed, status, (unsigned long long *)first);
  return (int)hipGetLastError();
}
extern "C" int md_launch_bgzf_plan(uint64_t nb, uint64_t len, uint64_t block, uint64_t stride, uint64_t *in_off, uint64_t *in_len,
                                   uint64_t *out_off, uint64_t *out_cap, hipStream_t stream) {
  if (nb == 0) return 0;
  hipLaunchKernelGGL(bgzf_plan_kernel, dim3(grid_of(nb, 256)), dim3(256), 0, stream, nb, len, block, stride, in_off, in_len, out_off, out_cap);
  return (int)hipGetLastError();
}
extern "C" int md_launch_bgzf_sizes(uint64_t nb, const uint64_t *in_len, const uint64_t *out_len, const int32_t *status, uint64_t *msize,
                                    int32_t *err, hipStream_t stream) {
  if (nb == 0) return 0;
  hipLaunchKernelGGL(bgzf_size_kernel, dim3(grid_of(nb, 256)), dim3(256), 0, stream, nb, in_len, out_len, status, msize, err);
  return (int)hipGetLastError();
}
extern "C" int md_launch_bgzf_pack(uint64_t nb, const uint8_t *src, const uint64_t *in_off, const uint64_t *in_len, const uint8_t *slots,
                                   const uint64_t *slot_off, const uint64_t *out_len, const int32_t *status, const uint64_t *moff,
                                   const uint32_t *crc, uint8_t *dst, hipStream_t stream) {
  hipLaunchKernelGGL(bgzf_pack_kernel, dim3((uint32_t)nb + 1), dim3(256), 0, stream, nb, src, in_off, in_len, slots, slot_off, out_len, status,
                     moff, crc, dst);
  return (int)hipGetLastError();
}
