// gz_spec.hip — the members of a GZip file that does NOT state their lengths (cat *.gz, WARC, mgzip, a BGZF file with one
// damaged BSIZE), found by speculation and verification on gfx950 (capi_gz_members.cpp: gzm_speculative).
// Every position that looks like a member's start is a candidate, the bytes between two candidates are a span, every
// plausible span is decoded as if it were a member, and a span is VERIFIED when that decode ends exactly where the next
// candidate begins with the CRC-32 and ISIZE found there.  The host then walks the file as libz reads it and takes the
// verified spans it stands on from this batch; everything else is its own one-member step.
//   mark_kernel      every byte position: 1f 8b 08, FLG without a reserved bit, 18 bytes left (the shortest member is 20).
//                    mark_kernel of gz_members.hip without the BC walk: 16 bytes a thread and step plus a 4-byte halo, the
//                    SWAR test for 1f, one bit per input byte, a count per workgroup
//   compact_kernel   the candidates' positions in order (the scan between the two is gz_members.hip's)
//   span_kernel      span k = [c_k, c_k+1), the last one ends with the file; header_kernel of gz_members.hip then parses
//                    each span as a member of that length: header status, body, the four bytes at its end as ISIZE guess
//   classify_kernel  rules (a) header, (b) a guess DEFLATE cannot reach, (c) a long body: the guess of a span that passes
//   room_kernel      rule (d) against the offsets scanned from those guesses; what the inflate launch gets per span
//   verify_kernel    after the inflate launch and gz_finish_kernel: the verified flag
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "mdeflate.h"

namespace md {
namespace gzs {

constexpr uint32_t kMarkThreads = 256;
constexpr uint32_t kMarkSteps = 4;
constexpr uint32_t kMarkSpan = kMarkThreads * kMarkSteps * 16;  // input bytes per workgroup
static_assert(kMarkSpan == gzm::kMarkSpanBytes, "the counts are scanned and sized as gz_members.hip's");

__global__ __launch_bounds__(kMarkThreads) void mark_kernel(const uint8_t *__restrict__ s, uint64_t len, uint32_t *__restrict__ bits,
                                                            uint32_t *__restrict__ cnt) {
  __shared__ uint32_t found;
  if (threadIdx.x == 0) found = 0;
  __syncthreads();
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
      const uint32_t x = w[k] ^ 0x1f1f1f1fu;
      has1f |= ((x - 0x01010101u) & ~x & 0x80808080u) != 0;
    }
    if (!has1f) continue;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
      const uint64_t p = c + k;
      if (p + kCandidateMin > len) break;
      const uint64_t two = ((uint64_t)w[(k >> 2) + 1] << 32) | w[k >> 2];
      const uint32_t sig = (uint32_t)(two >> (8 * (k & 3)));
      if ((sig & 0xe0ffffffu) != 0x00088b1fu) continue;
      atomicOr(&bits[p >> 5], 1u << (p & 31));
      atomicAdd(&found, 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = found;
}

__device__ __forceinline__ uint32_t wave_incl(uint32_t x, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if ((int)lane >= o) x += y;
  }
  return x;
}

// workgroup b: the bits mark_kernel's workgroup b set (kMarkSpan / 32 words, two a thread), in position order from base[b]
__global__ __launch_bounds__(kMarkThreads) void compact_kernel(uint64_t len, const uint32_t *__restrict__ bits, const uint64_t *__restrict__ base,
                                                               uint64_t *__restrict__ cpos) {
  __shared__ uint32_t wsum[kMarkThreads / 64];
  const uint64_t b0 = base[blockIdx.x];
  if (base[blockIdx.x + 1] == b0) return;  // (uniform: most spans hold no candidate)
  const uint64_t nwords = (len + 31) / 32;
  const uint64_t w0 = (uint64_t)blockIdx.x * (kMarkSpan / 32) + threadIdx.x * 2;
  uint32_t a[2] = {w0 < nwords ? bits[w0] : 0u, w0 + 1 < nwords ? bits[w0 + 1] : 0u};
  const uint32_t mine = __popc(a[0]) + __popc(a[1]);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t incl = wave_incl(mine, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint64_t k = b0 + incl - mine;
  for (uint32_t j = 0; j < wave; j++) k += wsum[j];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    while (a[h]) {
      const uint32_t bit = __builtin_ctz(a[h]);
      a[h] &= a[h] - 1;
      cpos[k++] = (w0 + h) * 32 + bit;
    }
  }
}

__global__ void span_kernel(uint64_t C, const uint64_t *__restrict__ cpos, uint64_t len, uint64_t *__restrict__ mlen) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= C) return;
  mlen[k] = (k + 1 < C ? cpos[k + 1] : len) - cpos[k];
}

// *sum_body: the sum of all body lengths (the scan of body_len).  pass[k] = the guess of a span that rules (a) to (c) let
// through, else 0; flag[k] = its reason code << 1.
__global__ void classify_kernel(uint64_t C, const int32_t *__restrict__ hstatus, const uint64_t *__restrict__ body_len,
                                const uint64_t *__restrict__ guess, const uint64_t *__restrict__ sum_body, uint64_t long_min,
                                uint64_t *__restrict__ pass, uint8_t *__restrict__ flag) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= C) return;
  const uint64_t b = body_len[k], g = guess[k];
  uint32_t why = kSpanAdmitted;
  // (a) no member's header; (b) a stored block of 65 535 bytes costs 5, the best codes one bit for 258 bytes: nothing
  // expands 1 032-fold
  if (hstatus[k] != MD_OK || g > 1032 * b + 8) why = kSpanImplausible;
  // (c) the batch lasts as long as its longest stream on one pair of wavefronts (and no stream may pass the kernel's limit)
  else if (b > MD_MAX_INFLATE_IN || (b >= long_min && b * kLongShare >= *sum_body)) why = kSpanLong;
  pass[k] = why == kSpanAdmitted ? g : 0;
  flag[k] = (uint8_t)(why << 1);
}

// out_off: the exclusive sums of pass[].  (d) a span whose guess ends behind dst_cap is left out, so the launch never
// writes past dst_cap bytes of its output; a span left out by any rule gets no input, no room and offset 0.
__global__ void room_kernel(uint64_t C, const uint64_t *__restrict__ body_len, const uint64_t *__restrict__ pass, uint64_t dst_cap,
                            uint64_t *__restrict__ out_off, uint64_t *__restrict__ dec_len, uint64_t *__restrict__ out_cap,
                            uint8_t *__restrict__ flag) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= C) return;
  uint32_t why = flag[k] >> 1;
  if (why == kSpanAdmitted && (out_off[k] > dst_cap || pass[k] > dst_cap - out_off[k])) why = kSpanNoRoom;
  const bool in = why == kSpanAdmitted;
  if (!in) out_off[k] = 0;
  dec_len[k] = in ? body_len[k] : 0;
  out_cap[k] = in ? pass[k] : 0;
  flag[k] = (uint8_t)(why << 1);
}

// status / consumed / out_len as gz_finish_kernel leaves them: MD_OK there is a CRC-32 and an ISIZE that match behind the
// body's last byte, consumed = header + body + 8.  Verified: that trailer is the span's end.
__global__ void verify_kernel(uint64_t C, const uint64_t *__restrict__ mlen, const int32_t *__restrict__ hstatus,
                              const int32_t *__restrict__ status, const uint64_t *__restrict__ consumed, const uint64_t *__restrict__ out_len,
                              const uint64_t *__restrict__ pass, uint8_t *__restrict__ flag) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= C) return;
  const uint8_t f = flag[k];
  const bool ok = (f >> 1) == kSpanAdmitted && hstatus[k] == MD_OK && status[k] == MD_OK && consumed[k] == mlen[k] && out_len[k] == pass[k];
  flag[k] = (uint8_t)(f | (ok ? kSpanVerified : 0u));
}

}  // namespace gzs
}  // namespace md

using namespace md::gzs;
static inline uint32_t grid_of(uint64_t n, uint32_t threads) { return (uint32_t)((n + threads - 1) / threads); }

extern "C" int md_launch_gzs_mark(const uint8_t *src, uint64_t len, uint32_t *bits, uint32_t *cnt, hipStream_t stream) {
  if (len == 0) return 0;
  const hipError_t e = hipMemsetAsync(bits, 0, (len + 31) / 32 * 4, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(mark_kernel, dim3(grid_of(len, kMarkSpan)), dim3(kMarkThreads), 0, stream, src, len, bits, cnt);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzs_compact(uint64_t len, const uint32_t *bits, const uint64_t *base, uint64_t *cpos, hipStream_t stream) {
  if (len == 0) return 0;
  hipLaunchKernelGGL(compact_kernel, dim3(grid_of(len, kMarkSpan)), dim3(kMarkThreads), 0, stream, len, bits, base, cpos);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzs_spans(uint64_t C, const uint64_t *cpos, uint64_t len, uint64_t *mlen, hipStream_t stream) {
  if (C == 0) return 0;
  hipLaunchKernelGGL(span_kernel, dim3(grid_of(C, 256)), dim3(256), 0, stream, C, cpos, len, mlen);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzs_classify(uint64_t C, const int32_t *hstatus, const uint64_t *body_len, const uint64_t *guess,
                                      const uint64_t *sum_body, uint64_t long_min, uint64_t *pass, uint8_t *flag, hipStream_t stream) {
  if (C == 0) return 0;
  hipLaunchKernelGGL(classify_kernel, dim3(grid_of(C, 256)), dim3(256), 0, stream, C, hstatus, body_len, guess, sum_body, long_min, pass, flag);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzs_room(uint64_t C, const uint64_t *body_len, const uint64_t *pass, uint64_t dst_cap, uint64_t *out_off,
                                  uint64_t *dec_len, uint64_t *out_cap, uint8_t *flag, hipStream_t stream) {
  if (C == 0) return 0;
  hipLaunchKernelGGL(room_kernel, dim3(grid_of(C, 256)), dim3(256), 0, stream, C, body_len, pass, dst_cap, out_off, dec_len, out_cap, flag);
  return (int)hipGetLastError();
}
extern "C" int md_launch_gzs_verify(uint64_t C, const uint64_t *mlen, const int32_t *hstatus, const int32_t *status, const uint64_t *consumed,
                                    const uint64_t *out_len, const uint64_t *pass, uint8_t *flag, hipStream_t stream) {
  if (C == 0) return 0;
  hipLaunchKernelGGL(verify_kernel, dim3(grid_of(C, 256)), dim3(256), 0, stream, C, mlen, hstatus, status, consumed, out_len, pass, flag);
  return (int)hipGetLastError();
}
