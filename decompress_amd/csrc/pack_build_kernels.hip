// pack_build_kernels.hip — where the zlib streams of a git pack may begin, for gfx950 (md_pack_index_build; mdeflate.h,
// capi_pack_build.cpp).  A pack without an idx does not say where its objects lie: object k + 1 begins where
// the stream of object k ends.  The device breaks that chain as gz_spec.hip does for gzip members: every position that
// may begin a zlib stream is a candidate, the size query (inflate_count.hip) walks all of them as one batch, and the host
// follows the chain from byte 12 through the answers (pack_build.hpp).
//   mark_kernel    every byte position z of [lo, hi]: pack[z], pack[z + 1] pass the decoder's own test of a zlib header
//                  (open_stream's ZLIB branch).  16 bytes a lane and step plus one byte of halo; two lanes make one word of
//                  the bitmap between them (a shuffle, no atomic on memory), every word of the bitmap is written, and a
//                  count per workgroup goes to the scan.  The layout is gz_spec.hip's, so its compact_kernel takes it
//   inputs_kernel  what the size query gets per candidate: in_len = what lies between z and the trailer, at most
//                  MD_MAX_INFLATE_IN (in_off is the candidates' list itself)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "mdeflate.h"

namespace md {
namespace pkb {

constexpr uint32_t kMarkThreads = 256;
constexpr uint32_t kMarkSteps = 4;
constexpr uint32_t kMarkSpan = kMarkThreads * kMarkSteps * 16;  // input bytes per workgroup
static_assert(kMarkSpan == gzm::kMarkSpanBytes, "the counts are scanned and the bits compacted as gz_spec.hip's");

// s: the pack (16-byte aligned), len bytes; candidates lie in [lo, hi], hi + 1 < len
__global__ __launch_bounds__(kMarkThreads) void mark_kernel(const uint8_t *__restrict__ s, uint64_t len, uint64_t lo, uint64_t hi,
                                                            uint32_t *__restrict__ bits, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t found;
  if (threadIdx.x == 0) found = 0;
  __syncthreads();
  const uint64_t nwords = (len + 31) / 32;
  for (uint32_t step = 0; step < kMarkSteps; step++) {  // (every lane takes every step: the shuffle below needs its neighbour)
    const uint64_t c = (uint64_t)blockIdx.x * kMarkSpan + ((uint64_t)step * kMarkThreads + threadIdx.x) * 16;
    uint32_t w[5] = {0, 0, 0, 0, 0};  // bytes c .. c + 16, NUL behind the end
    if (c < len && len - c >= 17) {
      const uint4 v = *(const uint4 *)(s + c);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      w[4] = s[c + 16];
    } else if (c < len) {
#pragma unroll
      for (uint32_t k = 0; k < 17; k++)  // (unrolled: w[] stays in registers)
        if (c + k < len) w[k >> 2] |= (uint32_t)s[c + k] << (8 * (k & 3));
    }
    uint32_t m = 0;
    if (c <= hi && c + 15 >= lo) {
#pragma unroll
      for (uint32_t k = 0; k < 16; k++) {
        const uint32_t cmf = (w[k >> 2] >> (8 * (k & 3))) & 0xff, flg = (w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xff;
        const bool hit = (cmf & 0xf) == 8 && ((cmf << 8) + flg) % 31 == 0 && c + k >= lo && c + k <= hi;
        m |= (hit ? 1u : 0u) << k;
      }
    }
    const uint32_t upper = (uint32_t)__shfl_down((int)m, 1);
    if (!(threadIdx.x & 1) && (c >> 5) < nwords) bits[c >> 5] = m | upper << 16;
    if (m) atomicAdd(&found, (uint32_t)__popc(m));
  }
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = found;
}

__global__ void inputs_kernel(uint64_t C, const uint64_t *__restrict__ cpos, uint64_t end, uint64_t *__restrict__ in_len) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= C) return;
  const uint64_t room = end - cpos[k];  // (cpos[k] <= end - 6: mark_kernel's hi)
  in_len[k] = room < MD_MAX_INFLATE_IN ? room : MD_MAX_INFLATE_IN;
}

}  // namespace pkb
}  // namespace md

using namespace md::pkb;
static inline uint32_t grid_of(uint64_t n, uint32_t threads) { return (uint32_t)((n + threads - 1) / threads); }

extern "C" int md_launch_pkb_mark(const uint8_t *pack, uint64_t len, uint64_t lo, uint64_t hi, uint32_t *bits, uint32_t *cnt, hipStream_t stream) {
  if (len == 0) return 0;
  hipLaunchKernelGGL(mark_kernel, dim3(grid_of(len, kMarkSpan)), dim3(kMarkThreads), 0, stream, pack, len, lo, hi, bits, cnt);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pkb_inputs(uint64_t C, const uint64_t *cpos, uint64_t end, uint64_t *in_len, hipStream_t stream) {
  if (C == 0) return 0;
  hipLaunchKernelGGL(inputs_kernel, dim3(grid_of(C, 256)), dim3(256), 0, stream, C, cpos, end, in_len);
  return (int)hipGetLastError();
}
