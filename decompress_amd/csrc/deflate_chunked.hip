// deflate_chunked.hip — the hash chains of ONE long stream on the whole chip (capi.cpp link_segments).
//
// deflate_link_kernel gives a stream one workgroup: the head table is 128 KiB of LDS, so one CU, ~0.8 ms per MiB.  In a
// batch of one that leaves 255 CUs idle.  link[p] only depends on the 32 767 positions in front of p (what lies further
// back is written as 0, and the matcher never takes a head beyond MAX_DIST), so the stream is cut into segments of S
// positions and segment k is one workgroup: it first inserts the 32 KiB in front of kS into its own head table without
// writing anything, then inserts and writes [kS, (k + 1)S).  link[] is the one pass's, position for position, and so is
// everything the match kernel and the sequential kernel do with it.  The segment that holds p_end - 1 hands over the tail
// heads (H7): its table holds every position of the last 32 KiB in front of len - 3, and a head further back is never a
// candidate.  Warm-up cost: 32 KiB / S more insertions (S = 256 KiB: an eighth).
#include "deflate_link.hpp"

namespace md {
namespace defl {

// one stream (stream 0 of the front workspace's plan); workgroup b takes segments b, b + gridDim.x, ... (a 1-D grid of
// at most one workgroup per CU)
__global__ __launch_bounds__(LW *kWave) void deflate_link_chunked_kernel(const uint8_t *__restrict__ in,
                                                                         const uint64_t *__restrict__ in_off,
                                                                         const uint64_t *__restrict__ in_len,
                                                                         const uint32_t *__restrict__ p_end_a,
                                                                         const uint64_t *__restrict__ slot,
                                                                         uint32_t *__restrict__ link, uint32_t *__restrict__ tail,
                                                                         const uint32_t *__restrict__ flags, uint32_t seg,
                                                                         uint32_t nseg) {
  __shared__ uint32_t head[HASH_SIZE];  // absolute position, 0 = NIL
  __shared__ uint32_t gmin_all[LW][kWave];
  __shared__ uint32_t turn;
  const uint32_t wv = threadIdx.x / kWave;
  if (flags[0]) return;
  const uint32_t p_end = p_end_a[0];
  const uint64_t l64 = in_len[0];
  const uint32_t slen = l64 > MD_MAX_STREAM ? 0u : (uint32_t)l64;
  if (slen < 4) return;  // (the host sends no such stream)
  const uint8_t *src = in + in_off[0];
  uint32_t *lk = link + slot[0];
  for (uint32_t k = blockIdx.x; k < nseg; k += gridDim.x) {  // (uniform over the workgroup)
    const uint32_t wlo = k * seg;
    if (wlo >= p_end) break;
    const uint32_t hi = p_end - wlo > seg ? wlo + seg : p_end;
    const uint32_t lo = wlo > (uint32_t)WSIZE ? wlo - (uint32_t)WSIZE : 0u;
    link_insert<false>(head, gmin_all[wv], &turn, src, slen, p_end, lo, wlo, hi, lk, MD_MATCHER_DE, 0u);
    __syncthreads();
    if (hi == p_end) link_tail(head, src, slen, MD_MATCHER_DE, tail);
  }
}

}  // namespace defl
}  // namespace md

// link[] / tail[] of stream 0 of the plan f (De matcher, p_end = len - 3 positions inserted ahead), segments of seg
// positions; the match kernel follows with md_launch_deflate_match
extern "C" int md_launch_link_chunked(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint32_t p_end,
                                      uint32_t seg, uint32_t cus, const md::defl::Front *f, hipStream_t stream) {
  using namespace md::defl;
  if (seg == 0 || p_end == 0) return (int)hipErrorInvalidValue;
  const uint32_t nseg = (p_end + seg - 1) / seg;
  const uint32_t grid = nseg < cus ? nseg : cus;
  hipLaunchKernelGGL(deflate_link_chunked_kernel, dim3(grid), dim3(LW * kWave), 0, stream, in, in_off, in_len, f->p_end,
                     f->slot, f->link, (uint32_t *)f->tail, f->flags, seg, nseg);
  return (int)hipGetLastError();
}
