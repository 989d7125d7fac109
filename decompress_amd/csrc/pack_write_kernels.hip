// pack_write_kernels.hip — making the deltas of a git pack on the device (md_pack_delta_batch_*; mdeflate.h),
// for gfx950.  The delta of a target against a base is defined byte for byte in mdeflate.h; tests/pack_delta_model.py is
// that definition in Python.
//
//   index_kernel   one thread per 16-byte block of every DISTINCT base of the call: the block's hash picks a slot of the
//                  base's table, atomicMin leaves the lowest block index there (the tables are preset to all ones)
//   delta_kernel   one wavefront per (base, target) pair: pack_delta_walk.hpp's walk with the writer on
//   assemble_kernel md_pack_write: every object's header bytes and compressed stream to its offset of the pack
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "copy_bytes.hpp"
#include "internal.hpp"
#include "mdeflate.h"
#include "pack_delta_walk.hpp"

namespace md {
namespace pkw {

__global__ __launch_bounds__(256) void index_kernel(uint32_t nbases, uint64_t blocks, const Base *__restrict__ bases,
                                                    const uint8_t *__restrict__ src, uint32_t *__restrict__ tables) {
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < blocks; t += (uint64_t)gridDim.x * 256) {
    // the base whose blocks hold t: the last one with first_block <= t (a base without blocks shares its neighbour's first_block
    // and is passed over, as the search keeps the last)
    uint32_t lo = 0, hi = nbases;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (bases[mid].first_block <= t) lo = mid;
      else hi = mid;
    }
    const Base b = bases[lo];
    const uint32_t j = (uint32_t)(t - b.first_block);
    const uint32_t slot = hash_block(load_block(src + b.off + (uint64_t)j * kBlock)) >> (32 - b.bits);
    atomicMin(tables + b.table_off + slot, j);
  }
}

// One wavefront per pair (the walk and its steps: pack_delta_walk.hpp).  The first op that would pass out_cap ends the pair
// with MD_UNEXPECTED_END_OF_OUTPUT and out_len 0.
__global__ __launch_bounds__(kWave) void delta_kernel(uint32_t count, const Pair *__restrict__ pairs, const uint8_t *__restrict__ src,
                                                      const uint32_t *__restrict__ tables, uint8_t *__restrict__ dst,
                                                      uint64_t *__restrict__ out_len, int32_t *__restrict__ status) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t d = blockIdx.x; d < count; d += gridDim.x) {
    const Pair row = pairs[d];
    bool full;
    const uint64_t o = delta_walk<true>(row, src, tables, dst + row.out_off, lane, &full);
    if (lane == 0) {
      out_len[d] = full ? 0 : o;
      status[d] = full ? MD_UNEXPECTED_END_OF_OUTPUT : MD_OK;
    }
  }
}

// md_pack_write: object i of the pack is its head_len[i] header bytes (head + kHeaderMax i) and its stream of zlen[i] bytes
// from slots + slot_off[i], at pack + offset[i].  One workgroup of 256 threads an object.
__global__ __launch_bounds__(256) void assemble_kernel(uint32_t n, const uint64_t *__restrict__ offset, const uint8_t *__restrict__ head,
                                                       const uint8_t *__restrict__ head_len, const uint8_t *__restrict__ slots,
                                                       const uint64_t *__restrict__ slot_off, const uint64_t *__restrict__ zlen,
                                                       uint8_t *__restrict__ pack) {
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t h = head_len[i];
    uint8_t *o = pack + offset[i];
    if (threadIdx.x < h) o[threadIdx.x] = head[kHeaderMax * i + threadIdx.x];
    copy_bytes(o + h, slots + slot_off[i], zlen[i]);
  }
}

}  // namespace pkw
}  // namespace md

using namespace md::pkw;
constexpr uint32_t kMaxWaveGrid = 1u << 20;  // wavefronts of a launch that strides over its work (as pack_kernels.hip's)
constexpr uint64_t kMaxIndexGrid = 1u << 20;

extern "C" int md_launch_pkw_index(uint32_t nbases, uint64_t blocks, const md::pkw::Base *bases, const uint8_t *src, uint32_t *tables,
                                   hipStream_t stream) {
  if (nbases == 0 || blocks == 0) return 0;
  const uint64_t groups = (blocks + 255) / 256;
  hipLaunchKernelGGL(index_kernel, dim3((uint32_t)(groups < kMaxIndexGrid ? groups : kMaxIndexGrid)), dim3(256), 0, stream, nbases, blocks, bases, src,
                     tables);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pkw_delta(uint32_t count, const md::pkw::Pair *pairs, const uint8_t *src, const uint32_t *tables, uint8_t *dst,
                                   uint64_t *out_len, int32_t *status, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(delta_kernel, dim3(count < kMaxWaveGrid ? count : kMaxWaveGrid), dim3(kWave), 0, stream, count, pairs, src, tables, dst, out_len,
                     status);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pkw_assemble(uint32_t n, const uint64_t *offset, const uint8_t *head, const uint8_t *head_len, const uint8_t *slots,
                                      const uint64_t *slot_off, const uint64_t *zlen, uint8_t *pack, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(assemble_kernel, dim3(n < kMaxWaveGrid ? n : kMaxWaveGrid), dim3(256), 0, stream, n, offset, head, head_len, slots, slot_off, zlen,
                     pack);
  return (int)hipGetLastError();
}
