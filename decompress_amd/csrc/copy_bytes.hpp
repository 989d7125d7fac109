// copy_bytes.hpp — the copy loop of the kernels that assemble a file from pieces, one workgroup of 256 threads per piece
// (bgzf_pack_kernel of gz_members.hip, join_kernel of deflate_spans.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace md {

// n bytes a -> o, 256 threads: 16-byte stores on o's alignment, a read with unaligned 16-byte loads
__device__ __forceinline__ void copy_bytes(uint8_t *__restrict__ o, const uint8_t *__restrict__ a, uint64_t n) {
  const uint64_t head = (16 - ((uintptr_t)o & 15)) & 15, h1 = head < n ? head : n;
  for (uint64_t k = threadIdx.x; k < h1; k += 256) o[k] = a[k];
  const uint64_t body = (n - h1) & ~(uint64_t)15;
  for (uint64_t k = h1 + (uint64_t)threadIdx.x * 16; k < h1 + body; k += 256 * 16) {
    uint4 v;
    __builtin_memcpy(&v, a + k, 16);
    *reinterpret_cast<uint4 *>(o + k) = v;
  }
  for (uint64_t k = h1 + body + threadIdx.x; k < n; k += 256) o[k] = a[k];
}

// the same by one wavefront (apply_kernel and repeats_kernel of pack_kernels.hip): lane = 0 .. 63
__device__ __forceinline__ void copy_bytes_wave(uint8_t *__restrict__ o, const uint8_t *__restrict__ a, uint64_t n, uint32_t lane) {
  const uint64_t head = (16 - ((uintptr_t)o & 15)) & 15, h1 = head < n ? head : n;
  if (lane < h1) o[lane] = a[lane];
  const uint64_t body = (n - h1) & ~(uint64_t)15;
  for (uint64_t k = h1 + (uint64_t)lane * 16; k < h1 + body; k += 64 * 16) {
    uint4 v;
    __builtin_memcpy(&v, a + k, 16);
    *reinterpret_cast<uint4 *>(o + k) = v;
  }
  const uint64_t t = h1 + body + lane;
  if (t < n) o[t] = a[t];
}

}  // namespace md
