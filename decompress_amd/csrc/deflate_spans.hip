// deflate_spans.hip — ONE RFC 1951 / 1950 / 1952 stream written as joined spans on gfx950: the kernels behind
// md_deflate_spans_* (capi_deflate_spans.cpp).  The text is cut into spans, every span is a stream of one deflate
// launch, and the bodies are joined the way pigz joins them: the closing block of every span but the last loses its BFINAL
// bit and is followed by an empty stored block (0 00, zero bits up to the byte, 00 00 FF FF), so a span ends on a byte.
//   plan_kernel   span i of the text -> stream i of the deflate launch, slots of fixed stride; a slot holds exactly the
//                 span's stored form, so a body that does not fit it has lost against that form already.  Primed spans:
//                 a second set of descriptors for the deflate launch alone - the stream is the span with the w = min(start,
//                 32 768) bytes in front of it, and it begins to emit at w (SeqArgs::first); everything that handles the
//                 text itself keeps the span's own offset and length
//   adler_kernel  the Adler-32 of every span whose body did not fit its slot, from the text: the encoder's word for such a
//                 span is not the whole span's when the batch went in slices of positions and the slot ran out early
//   size_kernel   per span the joined form J or the stored form S (S exactly when J is strictly longer), its length, the
//                 count of stored spans and the encoder's errors
//   join_kernel   one workgroup per span copies the body to its final offset (16-byte stores on the destination's
//                 alignment), clears bit h and writes the marker - or writes the stored blocks straight from the text; one
//                 more workgroup writes the header and the trailer: the spans' checksums fold into the stream's without an
//                 order (Adler-32: sums mod 65 521; CRC-32: crc_i * x^(8 * bytes behind span i), XOR-ed), a wave reduction
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "copy_bytes.hpp"
#include "gz_crc.hpp"
#include "internal.hpp"
#include "mdeflate.h"

namespace md {
namespace spn {

__global__ void plan_kernel(uint64_t n, uint64_t len, uint64_t span, uint64_t stride, uint64_t *__restrict__ in_off,
                            uint64_t *__restrict__ in_len, uint64_t *__restrict__ out_off, uint64_t *__restrict__ out_cap,
                            uint64_t *__restrict__ x_off, uint64_t *__restrict__ x_len, uint32_t *__restrict__ first) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t at = i * span, m = len - at < span ? len - at : span;
  in_off[i] = at;
  in_len[i] = m;
  out_off[i] = i * stride;
  out_cap[i] = stored_size(m);
  if (first) {  // primed: the stream of the deflate launch
    const uint64_t w = at < kPrime ? at : kPrime;
    x_off[i] = at - w;
    x_len[i] = w + m;
    first[i] = (uint32_t)w;
  }
}

// bytes of the marker behind a joined span whose closing block ends at bit e: the three header bits 0 00 go into the last
// byte where it has room for them
__device__ __forceinline__ uint32_t marker_len(uint64_t e) { return ((8 - (e & 7)) & 7) >= 3 ? 4u : 5u; }
// e lies in the body's last byte and h in front of it: what join_kernel relies on before it touches a byte
__device__ __forceinline__ bool tail_fits(uint64_t h, uint64_t e, uint64_t body) { return h < e && (e + 7) / 8 == body; }

// Span i's form and size: true = joined.  (A body that overflowed its slot of stored_size bytes is longer than the stored form.)
__device__ __forceinline__ bool span_form(const Spans &s, uint64_t i, uint64_t *size) {
  const uint64_t m = s.in_len[i], stored = stored_size(m), body = s.out_len[i], h = s.tail[2 * i], e = s.tail[2 * i + 1];
  uint64_t joined = ~0ull;
  if (s.status[i] == MD_OK && tail_fits(h, e, body)) joined = i + 1 < s.n ? body + marker_len(e) : body;
  *size = joined <= stored ? joined : stored;
  return joined <= stored;
}

__global__ void size_kernel(const Spans s) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n) return;
  const int st = s.status[i];
  // a span's own status (MD_QUEUE_FULL) is the call's; a call-level error of a span (negative) or a tail that does not fit
  // its body fails the call
  if (st > 0 && st != MD_UNEXPECTED_END_OF_OUTPUT) atomicMax(s.err, st);
  if (st < 0) atomicMin(s.err + 1, st);
  if (st == MD_OK && !tail_fits(s.tail[2 * i], s.tail[2 * i + 1], s.out_len[i])) atomicMin(s.err + 1, (int)MD_E_HIP);
  uint64_t size;
  if (!span_form(s, i, &size)) atomicAdd((unsigned long long *)s.stored, 1ull);
  s.size[i] = size;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint64_t wave_add(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

constexpr uint64_t kAdlerMod = 65521;

// Adler-32 of span i from the text, for the spans whose body did not fit (they go out stored): one workgroup of 256
// threads, 16 bytes a thread and step.  A chunk at offset x of the span's m bytes with byte sum t1 and sum of k * byte_k tk
// adds t1 to A and (m - x) t1 - tk to B; A = 1 + the sum, B = m + the sum.
__global__ __launch_bounds__(256) void adler_kernel(const Spans s, const uint8_t *__restrict__ src, uint32_t *__restrict__ adler) {
  const uint64_t i = blockIdx.x;
  if (s.status[i] != MD_UNEXPECTED_END_OF_OUTPUT) return;
  const uint8_t *p = src + s.in_off[i];
  const uint64_t m = s.in_len[i];
  uint64_t a = 0, b = 0;
  for (uint64_t x = (uint64_t)threadIdx.x * 16; x < m; x += 256 * 16) {
    uint32_t w[4] = {0, 0, 0, 0};  // (the last chunk: zeros behind the span's end add nothing)
    if (x + 16 <= m) __builtin_memcpy(w, p + x, 16);
    else {
#pragma unroll
      for (uint32_t k = 0; k < 16; k++)
        if (x + k < m) w[k >> 2] |= (uint32_t)p[x + k] << (8 * (k & 3));
    }
    uint32_t t1 = 0, tk = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      t1 = __builtin_amdgcn_udot4(w[q], 0x01010101u, t1, false);
      tk = __builtin_amdgcn_udot4(w[q], 0x03020100u + 0x04040404u * q, tk, false);
    }
    a += t1;  // (at most 255 * 2^32)
    b = (b + ((m - x) % kAdlerMod) * t1 + kAdlerMod - tk) % kAdlerMod;  // (tk <= 30 600 < 65 521)
  }
  a %= kAdlerMod;
  __shared__ uint64_t part[2][4];
  a = wave_add(a), b = wave_add(b);
  if ((threadIdx.x & 63) == 0) part[0][threadIdx.x >> 6] = a, part[1][threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = (1 + part[0][0] + part[0][1] + part[0][2] + part[0][3]) % kAdlerMod;
    b = (m + part[1][0] + part[1][1] + part[1][2] + part[1][3]) % kAdlerMod;
    adler[i] = (uint32_t)(b << 16 | a);
  }
}
// Adler-32 of the text from the spans' (lane < 64).  With s_i = a_i - 1: A = 1 + sum s_i, B = len + sum [(b_i - len_i) +
// (len - end_i) s_i], all mod 65 521 - every term stands for itself, so the lanes take spans in turn and add up.
__device__ uint32_t adler_fold(const Spans &s, uint32_t lane) {
  uint64_t a = 0, b = 0;
  for (uint64_t i = lane; i < s.n; i += 64) {
    const uint64_t ai = s.adler[i] & 0xffff, bi = s.adler[i] >> 16, m = s.in_len[i], behind = s.len - (s.in_off[i] + m);
    const uint64_t si = (ai + kAdlerMod - 1) % kAdlerMod;
    a = (a + si) % kAdlerMod;
    b = (b + bi + kAdlerMod - m % kAdlerMod + (behind % kAdlerMod) * si) % kAdlerMod;
  }
  a = (1 + wave_add(a)) % kAdlerMod;
  b = (s.len % kAdlerMod + wave_add(b)) % kAdlerMod;
  return (uint32_t)(b << 16 | a);
}
// CRC-32 of the text from the spans' (lane < 64): crc(A || B) = crc(A) * x^(8 |B|) xor crc(B), gz_crc.hpp
__device__ uint32_t crc_fold(const Spans &s, uint32_t lane) {
  uint32_t c = 0;
  for (uint64_t i = lane; i < s.n; i += 64) c ^= gz::gf_mul(gz::gf_xpow8(s.len - (s.in_off[i] + s.in_len[i])), s.crc[i]);
  return wave_xor(c);
}

__global__ __launch_bounds__(256) void join_kernel(const Frame f, const Spans s, const uint8_t *__restrict__ src,
                                                   const uint8_t *__restrict__ slots, uint8_t *__restrict__ dst, uint64_t dst_cap,
                                                   uint64_t *__restrict__ written, int32_t *__restrict__ status,
                                                   uint32_t *__restrict__ checksum) {
  const uint64_t i = blockIdx.x, body_len = s.off[s.n], total = f.hdr_len + body_len + trailer_len(f.format);
  const bool fits = total <= dst_cap;  // (else nothing is written: no byte of dst lies behind dst_cap)
  if (i == s.n) {  // header, trailer and the call's three result words
    if (threadIdx.x >= 64) return;
    const uint32_t sum = f.format == MD_FORMAT_GZIP ? crc_fold(s, threadIdx.x) : adler_fold(s, threadIdx.x);
    if (fits) {
      for (uint32_t k = threadIdx.x; k < f.hdr_len; k += 64) dst[k] = f.hdr[k];
      uint8_t *t = dst + f.hdr_len + body_len;
      // Zl.Def: Adler-32, big-endian; Gz.Def: CRC-32, then the input size mod 2^32, little-endian
      if (f.format == MD_FORMAT_ZLIB && threadIdx.x < 4) t[threadIdx.x] = (uint8_t)(sum >> (24 - 8 * threadIdx.x));
      if (f.format == MD_FORMAT_GZIP && threadIdx.x < 8)
        t[threadIdx.x] = (uint8_t)((threadIdx.x < 4 ? sum : (uint32_t)s.len) >> (8 * (threadIdx.x & 3)));
    }
    if (threadIdx.x == 0) {
      *written = total;
      *status = s.err[1] ? s.err[1] : s.err[0] ? s.err[0] : fits ? MD_OK : MD_UNEXPECTED_END_OF_OUTPUT;
      *checksum = sum;
    }
    return;
  }
  if (!fits) return;
  uint8_t *o = dst + f.hdr_len + s.off[i];
  const uint64_t m = s.in_len[i];
  const bool last = i + 1 == s.n;
  uint64_t size;
  if (span_form(s, i, &size)) {
    const uint8_t *b = slots + s.slot_off[i];
    const uint64_t body = s.out_len[i];
    copy_bytes(o, b, body);
    if (last) return;
    __syncthreads();  // (the byte with bit h has been written: the one store that follows is the later one)
    if (threadIdx.x == 0) {
      const uint64_t h = s.tail[2 * i], e = s.tail[2 * i + 1];
      o[h >> 3] = b[h >> 3] & (uint8_t)~(1u << (h & 7));  // BFINAL of the closing block
      // 0 00: three zero bits, then zero bits up to the byte - the encoder's pad bits are zero, so that is a byte of its
      // own only where the last one has no room; then LEN 0, NLEN ffff
      uint64_t p = body;
      if (marker_len(e) == 5) o[p++] = 0;
      o[p] = 0, o[p + 1] = 0, o[p + 2] = 0xff, o[p + 3] = 0xff;
    }
    return;
  }
  // stored: blocks of at most 65 535 bytes, BFINAL on the last block of the last span
  const uint64_t nb = stored_blocks(m);
  for (uint64_t k = 0; k < nb; k++) {
    const uint64_t at = k * kStoredMax;
    const uint32_t ln = (uint32_t)(m - at < kStoredMax ? m - at : kStoredMax);
    uint8_t *q = o + at + 5 * k;
    if (threadIdx.x < 5) {
      const uint32_t t = threadIdx.x;
      q[t] = t == 0 ? (uint8_t)(last && k + 1 == nb) : (uint8_t)((t < 3 ? ln : ~ln) >> (8 * ((t - 1) & 1)));
    }
    copy_bytes(q + 5, src + s.in_off[i] + at, ln);
  }
}

}  // namespace spn
}  // namespace md

using namespace md::spn;
static inline uint32_t grid_of(uint64_t n, uint32_t threads) { return (uint32_t)((n + threads - 1) / threads); }

extern "C" int md_launch_spans_plan(uint64_t n, uint64_t len, uint64_t span, uint64_t stride, uint64_t *in_off, uint64_t *in_len,
                                    uint64_t *out_off, uint64_t *out_cap, uint64_t *x_off, uint64_t *x_len, uint32_t *first,
                                    hipStream_t stream) {
  hipLaunchKernelGGL(plan_kernel, dim3(grid_of(n, 256)), dim3(256), 0, stream, n, len, span, stride, in_off, in_len, out_off, out_cap, x_off,
                     x_len, first);
  return (int)hipGetLastError();
}
extern "C" int md_launch_spans_adler(const Spans *s, const uint8_t *src, uint32_t *adler, hipStream_t stream) {
  hipLaunchKernelGGL(adler_kernel, dim3((uint32_t)s->n), dim3(256), 0, stream, *s, src, adler);
  return (int)hipGetLastError();
}
extern "C" int md_launch_spans_sizes(const Spans *s, hipStream_t stream) {
  hipLaunchKernelGGL(size_kernel, dim3(grid_of(s->n, 256)), dim3(256), 0, stream, *s);
  return (int)hipGetLastError();
}
extern "C" int md_launch_spans_join(const Frame *f, const Spans *s, const uint8_t *src, const uint8_t *slots, uint8_t *dst, uint64_t dst_cap,
                                    uint64_t *written, int32_t *status, uint32_t *checksum, hipStream_t stream) {
  hipLaunchKernelGGL(join_kernel, dim3((uint32_t)s->n + 1), dim3(256), 0, stream, *f, *s, src, slots, dst, dst_cap, written, status, checksum);
  return (int)hipGetLastError();
}
