// pack_search_kernels.hip — choosing the bases of a git pack's deltas on the device (md_pack_sketch_*, md_pack_delta_sizes_*,
// md_pack_choose_bases; mdeflate.h), for gfx950.  The sketch of an object is defined byte for byte in mdeflate.h;
// tests/pack_search_model.py is that definition in Python.
//
//   sketch_kernel  one wavefront per segment of kSegPositions positions of an object: lane l hashes the 16 bytes at every
//                  64th position from l and keeps four running minima; a wavefront reduction and four atomicMin fold the
//                  segment into the object's features (preset to all ones)
//   size_kernel    one wavefront per (base, target) pair: pack_delta_walk.hpp's walk with the writer off - the length and
//                  status md_pack_delta_batch_* would report, and no delta byte
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "mdeflate.h"
#include "pack_delta_walk.hpp"

namespace md {
namespace pks {

using pkw::kWave;

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (uint32_t m = kWave / 2; m; m >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, (int)m, (int)kWave);
    v = w < v ? w : v;
  }
  return v;
}

// Segment s: the positions [0, npos) from src + off, all of one object and every one with its 16 bytes inside the object
// (a window that reaches into the next segment's positions belongs to the segment in which it starts).  min does not
// depend on the order, so the features are a pure function of the object's bytes however it was cut.
__global__ __launch_bounds__(kWave) void sketch_kernel(uint32_t count, const Seg *__restrict__ segs, const uint8_t *__restrict__ src,
                                                       uint32_t *__restrict__ features) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t s = blockIdx.x; s < count; s += gridDim.x) {
    const Seg g = segs[s];
    const uint8_t *__restrict__ a = src + g.off;
    uint32_t f[kFeatures];
#pragma unroll
    for (uint32_t i = 0; i < kFeatures; i++) f[i] = pkw::kEmpty;
    for (uint32_t p = lane; p < g.npos; p += kWave) {  // (npos <= kSegPositions: no wrap)
      const uint32_t h = pkw::hash_block(pkw::load_block(a + p));
#pragma unroll
      for (uint32_t i = 0; i < kFeatures; i++) {
        const uint32_t v = (h ^ kSeeds[i]) * pkw::kHashMul;
        f[i] = v < f[i] ? v : f[i];
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < kFeatures; i++) {
      const uint32_t v = wave_min(f[i]);
      if (lane == 0) atomicMin(features + (uint64_t)kFeatures * g.obj + i, v);
    }
  }
}

// One wavefront per pair: out_len and status as delta_kernel's, nothing else written (out_off is not looked at).
__global__ __launch_bounds__(kWave) void size_kernel(uint32_t count, const pkw::Pair *__restrict__ pairs, const uint8_t *__restrict__ src,
                                                     const uint32_t *__restrict__ tables, uint64_t *__restrict__ out_len,
                                                     int32_t *__restrict__ status) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t d = blockIdx.x; d < count; d += gridDim.x) {
    const pkw::Pair row = pairs[d];
    bool full;
    const uint64_t o = pkw::delta_walk<false>(row, src, tables, nullptr, lane, &full);
    if (lane == 0) {
      out_len[d] = full ? 0 : o;
      status[d] = full ? MD_UNEXPECTED_END_OF_OUTPUT : MD_OK;
    }
  }
}

}  // namespace pks
}  // namespace md

constexpr uint32_t kMaxWaveGrid = 1u << 20;  // wavefronts of a launch that strides over its work (as pack_write_kernels.hip's)

extern "C" int md_launch_pks_sketch(uint32_t count, const md::pks::Seg *segs, const uint8_t *src, uint32_t *features, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(md::pks::sketch_kernel, dim3(count < kMaxWaveGrid ? count : kMaxWaveGrid), dim3(md::pkw::kWave), 0, stream, count, segs, src,
                     features);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pks_sizes(uint32_t count, const md::pkw::Pair *pairs, const uint8_t *src, const uint32_t *tables, uint64_t *out_len,
                                   int32_t *status, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(md::pks::size_kernel, dim3(count < kMaxWaveGrid ? count : kMaxWaveGrid), dim3(md::pkw::kWave), 0, stream, count, pairs, src,
                     tables, out_len, status);
  return (int)hipGetLastError();
}
