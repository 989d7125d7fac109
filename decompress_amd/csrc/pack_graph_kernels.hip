// pack_graph_kernels.hip — the object graph of a git pack on the device (md_pack_graph_build, md_pack_reachable; mdeflate.h),
// for gfx950.  The rules by which a commit, a tree and a tag name other objects are pack_graph.hpp's; the objects are read
// where a round of a read left them (capi_pack.cpp), behind the round's last apply launch.
//
//   tree_links_kernel    one wavefront per tree (below)
//   object_links_kernel  one thread per commit or tag: its tree and parents, or its one target
//   gather_kernel        one thread per edge: out of the objects' bound-sized slots into the compacted arrays, idx order
//   seed_kernel          the seeds of a walk marked
//   reach_step_kernel    one wavefront per object of the frontier: lanes stride its edges, a target marked first and
//                        with edges of its own goes to the next frontier (one atomicAdd a wavefront and 64 edges)
//   reach_finish_kernel  marks minus exclusions as bytes, and how many
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "mdeflate.h"
#include "pack_graph.hpp"
#include "pack_lookup.hpp"

namespace md {
namespace pkg {

constexpr uint32_t kWave = 64;

__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) { return (uint64_t)uniform32((uint32_t)(v >> 32)) << 32 | uniform32((uint32_t)v); }

// The name whose byte k is get(k) among the pack's: *to = its object or kNoLink, and the edge's flag for a target that
// has to be of type `wanted`.  The fan-out bounds the binary search to the names with the same first byte.
template <class Get>
__device__ __forceinline__ uint32_t lookup(const Links &l, Get get, uint32_t wanted, uint32_t *to) {
  const uint32_t b = get(0);
  uint64_t at = 0;
  const bool found = pk::find_name(l.names, b ? l.fan[b - 1] : 0, l.fan[b], get, &at);
  *to = found ? (uint32_t)at : pg::kNoLink;
  return pg::edge_flag(found, found ? l.type[at] : 0, wanted);
}

// One wavefront per tree.  Where an entry ends is only known from where it starts: its name runs to the first NUL, the 20
// bytes behind it may hold anything, the next entry starts behind them.  A step looks at kTreeWindow bytes from where the
// search for a NUL stands, an aligned dword a lane; four shuffles put byte 64 j + lane of the window into lane `lane`, and
// four ballots make the window's NULs 256 bits in scalar registers.  The scalar unit follows the chain - the first NUL at
// or behind the entry's start, then 21 bytes on - one shift and one find-first-set an entry, and hands entry e of the step
// to lane e, until the window or the lanes are used up.  The lanes then read their own entry (pack_graph.hpp's
// tree_entry_kind), look its 20 bytes up and write the edge.  A name that passes the window's end moves the window on
// with nothing to parse.  Any fault leaves the tree with no edge at all.
__global__ __launch_bounds__(kWave) void tree_links_kernel(Round r, Links l, const uint8_t *__restrict__ buf) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t t = blockIdx.x; t < r.count; t += gridDim.x) {
    const uint32_t q = uniform32(r.slot[t]), o = uniform32(r.obj[q]);
    const uint32_t size = uniform32((uint32_t)r.size[q]);  // (an object has at most MD_MAX_STREAM bytes)
    const uint64_t A = uniform64((uint64_t)(uintptr_t)(buf + r.off[q])), end = A + size, slot0 = uniform64(l.slot_off[o]);
    const uint8_t *__restrict__ a = (const uint8_t *)(uintptr_t)A;
    const uint32_t bound = size / (uint32_t)pg::kMinEntry;
    bool bad = false;
    uint32_t cnt = 0;
    if (uniform32((uint32_t)r.status[q]) == (uint32_t)MD_OK && size != 0) {
      bad = !pg::tree_walkable(size, size > pg::kNameBytes ? uniform32(a[size - pg::kNameBytes - 1]) : 1u);
      uint32_t s = 0, scan = 0;  // the entry that is next, and where the search for its NUL goes on
      while (!bad && s < size) {
        if (size - s < pg::kMinEntry - 1) {
          bad = true;
          break;
        }
        const uint64_t g = A + scan, gb = g & ~(uint64_t)3, mine = gb + 4 * lane;
        // No dword without a byte of the tree is read, but the first and the last may hold up to 3 bytes in front of it and
        // behind it: a round's objects stand on 64 bytes from the buffer's start (slot_stride, capi_pack.cpp), so the first
        // does not begin in front of the buffer, and the buffer ends 64 bytes behind its last slot (scratch0 + max_scratch
        // + 64).  The masks below leave those bytes out.
        const uint32_t word = mine < end ? *(const uint32_t *)(uintptr_t)mine : 0u;
        uint64_t m[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
          const uint32_t w = (uint32_t)__shfl((int)word, (int)(16 * j + (lane >> 2)));
          m[j] = __ballot(gb + 64 * j + lane < end && ((w >> (8 * (lane & 3))) & 0xff) == 0);
        }
        uint32_t rel = (uint32_t)(g - gb), ne = 0, my_s = 0, my_nul = 0;
        while (ne < kWave && rel < kTreeWindow) {
          uint32_t j = rel >> 6;
          uint64_t mm = (j == 0 ? m[0] : j == 1 ? m[1] : j == 2 ? m[2] : m[3]) & (~0ull << (rel & 63));
          while (mm == 0 && ++j < 4) mm = j == 1 ? m[1] : j == 2 ? m[2] : m[3];
          if (mm == 0) break;  // the name's NUL lies beyond the window
          const uint32_t nul = (uint32_t)(gb + 64 * j + (uint32_t)__builtin_ctzll(mm) - A);
          if (lane == ne) my_s = s, my_nul = nul;
          ne++;
          s = nul + 1 + (uint32_t)pg::kNameBytes;  // (at most size: the NUL at size - 21 is the last that can be found)
          if (size - s < pg::kMinEntry - 1) break;  // the tree's end, or spare bytes: the outer loop's to say
          rel = (uint32_t)(A + s - gb);
        }
        if (ne == 0) {  // a name longer than the window: on to the next one
          scan = (uint32_t)(gb + kTreeWindow - A);
          continue;
        }
        scan = s;
        uint32_t kind = pg::kTreeGitlink, to = pg::kNoLink;
        if (lane < ne) kind = pg::tree_entry_kind(a, my_s, my_nul);
        if (__ballot(kind == pg::kMalformed) != 0 || ne > bound - cnt) {
          bad = true;
          break;
        }
        if (lane < ne) {
          const uint8_t *nm = a + my_nul + 1;
          if (kind != pg::kTreeGitlink) kind |= lookup(l, [&](uint32_t k) { return (uint32_t)nm[k]; }, pg::wanted_type(kind, 0), &to);
          l.to[slot0 + cnt + lane] = to;
          l.kind[slot0 + cnt + lane] = (uint8_t)kind;
        }
        cnt += ne;
      }
    }
    if (lane == 0) l.deg[o] = bad ? 0 : cnt, l.bad[o] = bad;
  }
}

__global__ void object_links_kernel(Round r, Links l, const uint8_t *__restrict__ buf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.count) return;
  const uint32_t q = r.slot[i], o = r.obj[q];
  const uint64_t size = r.size[q], slot0 = l.slot_off[o];
  const uint8_t *__restrict__ a = buf + r.off[q];
  uint32_t deg = 0;
  bool bad = false;
  if (r.status[q] == MD_OK) {
    if (r.type[q] == 1) {
      bad = !pg::commit_walk(a, size, [&](uint64_t pos, uint32_t kind, const uint8_t *hex) {
        uint32_t to = pg::kNoLink;
        kind |= lookup(l, [&](uint32_t k) { return pg::hex_byte(hex, k); }, pg::wanted_type(kind, 0), &to);
        l.to[slot0 + pos] = to;
        l.kind[slot0 + pos] = (uint8_t)kind;
        deg = (uint32_t)pos + 1;
      });
    } else if (r.type[q] == 4) {  // (anything else has no links to read and no slot to write to)
      const uint32_t tag_type = pg::tag_target_type(a, size);
      bad = tag_type == 0;
      if (!bad) {
        uint32_t to = pg::kNoLink;
        const uint8_t *hex = a + 7;
        const uint32_t kind = pg::kTagTarget | lookup(l, [&](uint32_t k) { return pg::hex_byte(hex, k); }, tag_type, &to);
        l.to[slot0] = to;
        l.kind[slot0] = (uint8_t)kind;
        deg = 1;
      }
    }
  }
  l.deg[o] = bad ? 0 : deg;
  l.bad[o] = bad;
}

__global__ void gather_kernel(uint64_t n, uint64_t edges, const uint64_t *__restrict__ slot_off, const uint64_t *__restrict__ first,
                              const uint32_t *__restrict__ slot_to, const uint8_t *__restrict__ slot_kind, uint32_t *__restrict__ to,
                              uint8_t *__restrict__ kind) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= edges) return;
  uint64_t lo = 0, hi = n;  // the last object whose first edge is at or in front of e: it has one, first[n] = edges > e
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= e) lo = mid;
    else hi = mid;
  }
  const uint64_t from = slot_off[lo] + (e - first[lo]);
  to[e] = slot_to[from];
  kind[e] = slot_kind[from];
}

__global__ void seed_kernel(uint32_t count, const uint32_t *__restrict__ seed, uint32_t *__restrict__ mark) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < count) mark[seed[k]] = 1;
}

__global__ __launch_bounds__(kWave) void reach_step_kernel(Reach r, const uint32_t *__restrict__ frontier, uint32_t count) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t f = blockIdx.x; f < count; f += gridDim.x) {
    const uint32_t o = uniform32(frontier[f]);
    const uint64_t b = uniform64(r.first[o]), e = uniform64(r.first[o + 1]);
    for (uint64_t i0 = b; i0 < e; i0 += kWave) {
      const uint64_t i = i0 + lane;
      const uint32_t t = i < e ? r.to[i] : pg::kNoLink;
      bool push = false;  // the one lane that marks t, if t has edges to follow
      if (t != pg::kNoLink && atomicExch(&r.mark[t], 1u) == 0) push = r.first[t] != r.first[t + 1];
      const uint64_t m = __ballot(push);
      if (m != 0) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(r.next_len, (uint32_t)__popcll(m));
        base = uniform32(base);
        if (push) r.next[base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = t;
      }
    }
  }
}

__global__ void reach_finish_kernel(uint64_t n, const uint32_t *__restrict__ mark, const uint32_t *__restrict__ excluded, uint8_t *__restrict__ out,
                                    uint32_t *__restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n && mark[i] != 0 && !(excluded && excluded[i] != 0);
  if (i < n) out[i] = in;
  const uint64_t m = __ballot(in);
  if (m != 0 && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(count, (uint32_t)__popcll(m));
}

}  // namespace pkg
}  // namespace md

using namespace md::pkg;
static inline uint32_t grid_of(uint64_t n, uint32_t threads) { return (uint32_t)((n + threads - 1) / threads); }
constexpr uint32_t kMaxWaveGrid = 1u << 20;  // wavefronts of a launch that strides over its work

extern "C" int md_launch_pkg_tree_links(const md::pkg::Round *r, const md::pkg::Links *l, const uint8_t *buf, hipStream_t stream) {
  if (r->count == 0) return 0;
  hipLaunchKernelGGL(tree_links_kernel, dim3(r->count < kMaxWaveGrid ? r->count : kMaxWaveGrid), dim3(kWave), 0, stream, *r, *l, buf);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pkg_object_links(const md::pkg::Round *r, const md::pkg::Links *l, const uint8_t *buf, hipStream_t stream) {
  if (r->count == 0) return 0;
  hipLaunchKernelGGL(object_links_kernel, dim3(grid_of(r->count, 256)), dim3(256), 0, stream, *r, *l, buf);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pkg_gather(uint64_t n, uint64_t edges, const uint64_t *slot_off, const uint64_t *first, const uint32_t *slot_to,
                                    const uint8_t *slot_kind, uint32_t *to, uint8_t *kind, hipStream_t stream) {
  if (edges == 0) return 0;
  hipLaunchKernelGGL(gather_kernel, dim3(grid_of(edges, 256)), dim3(256), 0, stream, n, edges, slot_off, first, slot_to, slot_kind, to, kind);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pkg_seed(uint32_t count, const uint32_t *seed, uint32_t *mark, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(seed_kernel, dim3(grid_of(count, 256)), dim3(256), 0, stream, count, seed, mark);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pkg_reach_step(const md::pkg::Reach *r, const uint32_t *frontier, uint32_t count, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(reach_step_kernel, dim3(count < kMaxWaveGrid ? count : kMaxWaveGrid), dim3(kWave), 0, stream, *r, frontier, count);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pkg_reach_finish(uint64_t n, const uint32_t *mark, const uint32_t *excluded, uint8_t *out, uint32_t *count,
                                          hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(reach_finish_kernel, dim3(grid_of(n, 256)), dim3(256), 0, stream, n, mark, excluded, out, count);
  return (int)hipGetLastError();
}
