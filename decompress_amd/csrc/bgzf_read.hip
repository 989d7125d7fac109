// bgzf_read.hip — byte ranges of a blocked GZip file on the device (md_bgzf_read; mdeflate.h), for gfx950.  The header
// walk, the inflate launch and the trailer check are the many-member reader's (md_launch_gzm_headers,
// md_inflate_batch_device, md_launch_gz_finish); what is here stands behind them.
//
//   verdict_kernel   one thread per member of the round: the first of the header's status, the decoder's, a body that did
//                    not end at the trailer, the trailer check's, and a member that is sound but not the one the index
//                    describes (its BC field states another length, its ISIZE another size)
//   gather_kernel    one wavefront per (range, 16 KiB segment of its bytes in this round) copies from the members' slots
//                    into the range (16-byte stores on the destination's alignment), and the range's status
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "mdeflate.h"

namespace md {
namespace bgr {

constexpr uint32_t kWave = 64;

__device__ __forceinline__ uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// BSIZE + 1 of the member m[0, len), whose header md::gz::rfc_header accepted (so the extra field, if FLG says there is
// one, lies inside len); 0 without a BC subfield
__device__ uint32_t stated_length(const uint8_t *__restrict__ m, uint64_t len) {
  if (len < 12 || !(m[3] & 4)) return 0;
  const uint32_t xlen = le16(m + 10);
  if (len - 12 < xlen) return 0;
  for (uint32_t q = 0; q + 4 <= xlen;) {
    const uint8_t *f = m + 12 + q;
    const uint32_t sl = le16(f + 2);
    if (q + 4 + sl > xlen) return 0;
    if (f[0] == 'B' && f[1] == 'C' && sl == 2) return le16(f + 4) + 1;
    q += 4 + sl;
  }
  return 0;
}

// The slot is as large as the index says the member's output is, so the decoder running out of it speaks about the
// index unless the member's own ISIZE agrees with it (then the member overran its ISIZE: md_gz_members_uncompress' word).
__global__ void verdict_kernel(uint32_t count, const uint8_t *__restrict__ blob, Round r) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const int32_t hs = r.hstatus[j], is = r.inf_status[j], fs = r.status[j];
  const uint64_t len = r.mlen[j], cap = r.cap[j];
  int32_t v;
  if (hs != MD_OK) v = hs;
  else if (is == MD_UNEXPECTED_END_OF_OUTPUT) v = r.isize[j] == cap ? MD_INVALID_SIZE : MD_INVALID_INDEX;
  else if (is != MD_OK) v = is;
  else if (r.inf_consumed[j] != r.body_len[j]) v = MD_INVALID_SIZE;
  else if (fs != MD_OK) v = fs;
  else v = stated_length(blob + r.mpos[j], len) != len || r.isize[j] != cap ? MD_INVALID_INDEX : MD_OK;
  r.verdict[j] = v;
}

// the member of the round that holds byte x of the output or is the last in front of it: the last j with u0[j] <= x
// (u0[0] <= x)
__device__ __forceinline__ uint32_t member_of(const uint64_t *__restrict__ u0, uint32_t count, uint64_t x) {
  uint32_t lo = 0, hi = count;  // u0[lo] <= x < u0[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (u0[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
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
  const uint64_t tail = h1 + body + lane;
  if (tail < n) o[tail] = a[tail];
}

// grid (ranges with bytes in this round, segments): wavefront (q, y) copies segments y, y + gridDim.y, .. of what range
// ids[q] has in this round; (q, 0) also looks at the verdicts of the range's members of this round.  Rounds go through the
// members in order and one wavefront a round writes status[i], so the first verdict that is not MD_OK to reach it is the
// first failing member's, and it stays.
__global__ __launch_bounds__(kWave) void gather_kernel(uint32_t count, Round r, uint32_t nr, const uint32_t *__restrict__ ids,
                                                       const uint64_t *__restrict__ off, const uint64_t *__restrict__ len,
                                                       const uint8_t *__restrict__ slots, uint8_t *__restrict__ dst,
                                                       const uint64_t *__restrict__ dst_off, int32_t *__restrict__ status) {
  const uint32_t q = blockIdx.x, lane = threadIdx.x;
  if (q >= nr) return;
  const uint64_t i = ids[q], L = len[i], o = off[i];
  const uint64_t lo = r.u0[0], hi = r.u0[count - 1] + r.cap[count - 1];  // the round's span of the output
  const uint64_t a = o > lo ? o : lo, b = o + L < hi ? o + L : hi;
  if (a >= b) return;
  if (blockIdx.y == 0) {
    const uint32_t ja = member_of(r.u0, count, a), jb = member_of(r.u0, count, b - 1);
    uint32_t bad = 0xffffffffu;
    for (uint32_t j = ja + lane; j <= jb; j += kWave)
      if (r.verdict[j] != MD_OK && j < bad) bad = j;
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t other = __shfl_xor(bad, d);
      bad = other < bad ? other : bad;
    }
    if (lane == 0 && bad != 0xffffffffu && status[i] == MD_OK) status[i] = r.verdict[bad];
  }
  const uint64_t nseg = (b - a + kGatherSegment - 1) / kGatherSegment;
  for (uint64_t s = blockIdx.y; s < nseg; s += gridDim.y) {
    uint64_t pos = a + s * kGatherSegment;
    const uint64_t end = b - pos < kGatherSegment ? b : pos + kGatherSegment;
    // (the members of a round that lie under one range follow each other without a gap: only empty ones were left out)
    for (uint32_t j = member_of(r.u0, count, pos); pos < end && j < count; j++) {
      const uint64_t u = r.u0[j], mend = u + r.cap[j], e = mend < end ? mend : end;
      if (r.verdict[j] == MD_OK) wave_copy(dst + dst_off[i] + (pos - o), slots + r.slot[j] + (pos - u), e - pos, lane);
      pos = e;
    }
  }
}

}  // namespace bgr
}  // namespace md

extern "C" int md_launch_bgr_verdict(uint32_t count, const uint8_t *blob, const md::bgr::Round *r, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(md::bgr::verdict_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, count, blob, *r);
  return (int)hipGetLastError();
}
extern "C" int md_launch_bgr_gather(uint32_t count, const md::bgr::Round *r, uint32_t nr, const uint32_t *ids, uint64_t longest,
                                    const uint64_t *off, const uint64_t *len, const uint8_t *slots, uint8_t *dst, const uint64_t *dst_off,
                                    int32_t *status, hipStream_t stream) {
  if (count == 0 || nr == 0 || longest == 0) return 0;
  const uint64_t nseg = (longest + md::bgr::kGatherSegment - 1) / md::bgr::kGatherSegment;
  hipLaunchKernelGGL(md::bgr::gather_kernel, dim3(nr, (uint32_t)(nseg < 4096 ? nseg : 4096)), dim3(md::bgr::kWave), 0, stream, count, *r, nr, ids,
                     off, len, slots, dst, dst_off, status);
  return (int)hipGetLastError();
}
