// pack_lookup.hpp — a 20-byte name among a pack's sorted names, for the kernels that follow one: the base of a REF_DELTA
// (pack_kernels.hip) and the targets of a commit, a tree or a tag (pack_graph_kernels.hip).  Device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace md {
namespace pk {

// The name whose byte k is get(k), k = 0 .. 19, among names[lo, hi) - 20 bytes each, ascending - by binary search: true and
// *at = its place, or false.  get may be asked for a byte more than once.
template <class Get>
__device__ __forceinline__ bool find_name(const uint8_t *__restrict__ names, uint64_t lo, uint64_t hi, Get get, uint64_t *at) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint8_t *nm = names + mid * 20;
    int c = 0;
    for (uint32_t k = 0; k < 20 && c == 0; k++) c = (int)nm[k] - (int)get(k);
    if (c == 0) {
      *at = mid;
      return true;
    }
    if (c < 0) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

}  // namespace pk
}  // namespace md
