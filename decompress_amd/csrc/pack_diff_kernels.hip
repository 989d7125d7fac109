// pack_diff_kernels.hip — trees of a git pack diffed on the device (md_pack_diff; mdeflate.h), for gfx950.  The rules - canonical
// mode, key order, what a pair of entries gives - are pack_diff.hpp's; the trees are read where a read that keeps its objects
// on the device left them (capi_pack.cpp), one level of the recursion a time (capi_pack_diff.cpp).
//
//   tree_table_kernel        one wavefront per distinct tree of the level: a row per entry, the count, the verdict (below)
//   tree_diff_kernel<kWrite>  one wavefront per pair: lanes stride A's rows and search B's by key, then stride B's rows and
//                            search A's for what only B has; one walk counts (records, bytes of names) or writes them
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "internal.hpp"
#include "mdeflate.h"
#include "pack_diff.hpp"
#include "pack_graph.hpp"

namespace md {
namespace pkd {

constexpr uint32_t kWave = 64;
using pkg::kTreeWindow;

__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) { return (uint64_t)uniform32((uint32_t)(v >> 32)) << 32 | uniform32((uint32_t)v); }

// One wavefront per tree.  The walk is tree_links_kernel's (pack_graph_kernels.hip): a step looks at kTreeWindow bytes from where
// the search for a NUL stands, an aligned dword a lane, four ballots make the window's NULs 256 bits in scalar registers, the
// scalar unit follows the chain of entry starts and hands entry e of the step to lane e.  The lanes then parse their own entry
// (pack_diff.hpp's entry_mode over pack_graph.hpp's rules) and write its row.  With all rows written, lanes stride the
// neighbouring rows e, e + 1 - whichever steps wrote them - and compare their keys: the tree is sorted iff every pair ascends.
// A tree that did not decode, cannot be walked or is not sorted has ok = 0 and no rows that count.
__global__ __launch_bounds__(kWave) void tree_table_kernel(Trees t, const uint8_t *buf) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t tr = blockIdx.x; tr < t.count; tr += gridDim.x) {
    const uint32_t size = uniform32((uint32_t)t.size[tr]);  // (an object has at most MD_MAX_STREAM bytes)
    const uint64_t A = uniform64((uint64_t)(uintptr_t)(buf + t.off[tr])), end = A + size;
    const uint8_t *a = (const uint8_t *)(uintptr_t)A;
    Row *rows = t.rows + uniform64(t.row_off[tr]);
    const uint32_t bound = size / (uint32_t)pg::kMinEntry;
    bool bad = uniform32((uint32_t)t.status[tr]) != (uint32_t)MD_OK;
    uint32_t cnt = 0;
    if (!bad && size != 0) {
      bad = !pg::tree_walkable(size, size > pg::kNameBytes ? uniform32(a[size - pg::kNameBytes - 1]) : 1u);
      uint32_t s = 0, scan = 0;  // the entry that is next, and where the search for its NUL goes on
      while (!bad && s < size) {
        if (size - s < pg::kMinEntry - 1) {
          bad = true;
          break;
        }
        const uint64_t g = A + scan, gb = g & ~(uint64_t)3, mine = gb + 4 * lane;
        // No dword without a byte of the tree is read; the first and the last may hold up to 3 bytes of a neighbour or of the
        // 64 bytes that the read's buffer has behind its objects (slot_stride, capi_pack.cpp).  The masks leave those bytes out.
        const uint32_t word = mine < end ? *(const uint32_t *)(uintptr_t)mine : 0u;
        uint64_t m[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
          const uint32_t w = (uint32_t)__shfl((int)word, (int)(16 * j + (lane >> 2)));
          m[j] = __ballot(gb + 64 * j + lane >= A && gb + 64 * j + lane < end && ((w >> (8 * (lane & 3))) & 0xff) == 0);
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
        uint32_t mode = pd::kDirMode;
        if (lane < ne) mode = pd::entry_mode(a, my_s, my_nul);
        if (__ballot(mode == 0) != 0 || ne > bound - cnt) {
          bad = true;
          break;
        }
        if (lane < ne) rows[cnt + lane] = Row{my_s, pd::entry_name(a, my_s), my_nul, mode};
        cnt += ne;
      }
    }
    __syncthreads();  // the rows are in memory for every lane of the wavefront
    bool unsorted = false;
    if (!bad)
      for (uint32_t e0 = 0; e0 + 1 < cnt; e0 += kWave) {
        const uint32_t e = e0 + lane;
        if (e + 1 < cnt) unsorted = unsorted || pd::key_compare(a, rows[e], a, rows[e + 1]) >= 0;
      }
    bad = bad || __ballot(unsorted) != 0;
    if (lane == 0) t.cnt[tr] = bad ? 0 : cnt, t.ok[tr] = !bad;
    __syncthreads();  // (the next tree's rows may stand where no lane still reads)
  }
}

// one side of a pair: the tree's bytes, its rows and their number, its object; the empty tree has no rows
struct Side {
  const uint8_t *bytes;
  const Row *rows;
  uint32_t n, obj;
};
__device__ __forceinline__ Side side_of(const Trees &t, const uint8_t *buf, uint32_t s) {
  Side x = {buf, t.rows, 0, pd::kNone};
  if (s != pd::kNone) {
    x.bytes = buf + uniform64(t.off[s]);
    x.rows = t.rows + uniform64(t.row_off[s]);
    x.n = uniform32(t.cnt[s]);
    x.obj = uniform32(t.obj[s]);
  }
  return x;
}

// the 20 bytes at b as five words of a record (they stand on no boundary in the tree)
__device__ __forceinline__ void name_words(uint32_t *w, const uint8_t *b) {
#pragma unroll
  for (uint32_t k = 0; k < 5; k++) w[k] = (uint32_t)b[4 * k] | (uint32_t)b[4 * k + 1] << 8 | (uint32_t)b[4 * k + 2] << 16 | (uint32_t)b[4 * k + 3] << 24;
}
// the graph's target of entry e of tree o
__device__ __forceinline__ uint32_t target(const Pairs &p, uint32_t o, uint32_t e) {
  const uint64_t at = p.first[o] + e;
  return at < p.first[o + 1] ? p.to[at] : pg::kNoLink;
}

static_assert(sizeof(md_tree_change) == 80 && offsetof(md_tree_change, kind) == 8 && offsetof(md_tree_change, a_mode) == 12 &&
                  offsetof(md_tree_change, a_obj) == 20 && offsetof(md_tree_change, name_len) == 28 && offsetof(md_tree_change, name_off) == 32 &&
                  offsetof(md_tree_change, a_name) == 40 && offsetof(md_tree_change, b_name) == 60,
              "a record is stored as 20 words");

// The rows of X, 64 a step, each searched for in Y.  kSecond = false: X is A - what is only there, and what matches and
// differs ('D', 'M', 'T'); true: X is B - what is only there ('A').  A record's slot within the pair comes from the ballot of
// the step and the records in front of it (recs), its name's place from a prefix sum of the step's name lengths (bytes).
template <bool kWrite, bool kSecond>
__device__ __forceinline__ void walk_side(const Side &X, const Side &Y, const Pairs &p, uint32_t q, uint32_t lane, uint32_t &recs, uint64_t &bytes) {
  for (uint32_t i0 = 0; i0 < X.n; i0 += kWave) {
    const uint32_t i = i0 + lane;
    uint32_t kind = 0, j = pd::kNone;
    Row rx = {0, 0, 0, 0}, ry = {0, 0, 0, 0};
    if (i < X.n) {
      rx = X.rows[i];
      j = pd::find_key(X.bytes, rx, Y.bytes, [&](uint32_t k) { return Y.rows[k]; }, Y.n);
      if (kSecond) {
        kind = j == pd::kNone ? (uint32_t)'A' : 0u;
      } else {
        if (j != pd::kNone) ry = Y.rows[j];
        kind = pd::classify(j != pd::kNone, rx.mode, ry.mode, j != pd::kNone && pd::same_name20(X.bytes + rx.nul + 1, Y.bytes + ry.nul + 1));
      }
    }
    const uint64_t m = __ballot(kind != 0);
    if (m == 0) continue;
    const uint32_t len = kind != 0 ? rx.nul - rx.name : 0;
    uint32_t inc = len;  // the name lengths summed up to this lane
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)inc, d);
      if (lane >= d) inc += v;
    }
    const uint32_t total = uniform32((uint32_t)__shfl((int)inc, kWave - 1));
    if (kWrite && kind != 0) {
      const uint32_t slot = recs + (uint32_t)__popcll(m & ((1ull << lane) - 1));
      const uint64_t place = p.name_first[q] + bytes + (inc - len);
      uint32_t w[20];
      w[0] = p.id[q], w[1] = p.parent[q];
      const bool dir = pd::is_dir(rx.mode);
      w[2] = kind | (dir ? pd::kFlagTree : 0u) << 8;
      w[7] = len, w[8] = (uint32_t)(p.name_base + place), w[9] = (uint32_t)((p.name_base + place) >> 32);
      const bool has_y = !kSecond && j != pd::kNone;
      // the side X is on, then the other one
      uint32_t mx = rx.mode, ox = target(p, X.obj, i), my = 0, oy = pg::kNoLink, nx[5], ny[5] = {0, 0, 0, 0, 0};
      name_words(nx, X.bytes + rx.nul + 1);
      if (has_y) {
        my = ry.mode, oy = target(p, Y.obj, j);
        name_words(ny, Y.bytes + ry.nul + 1);
      }
      w[3] = kSecond ? my : mx, w[4] = kSecond ? mx : my;
      w[5] = kSecond ? oy : ox, w[6] = kSecond ? ox : oy;
#pragma unroll
      for (uint32_t k = 0; k < 5; k++) w[10 + k] = kSecond ? ny[k] : nx[k], w[15 + k] = kSecond ? nx[k] : ny[k];
      uint32_t *o = (uint32_t *)(p.out + p.rec_first[q] + slot);
#pragma unroll
      for (uint32_t k = 0; k < 20; k++) o[k] = w[k];
      uint8_t *nm = p.names + place;
      for (uint32_t k = 0; k < len; k++) nm[k] = X.bytes[rx.name + k];
    }
    recs += (uint32_t)__popcll(m);
    bytes += total;
  }
}

template <bool kWrite>
__global__ __launch_bounds__(kWave) void tree_diff_kernel(Trees t, Pairs p, const uint8_t *buf) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t q = blockIdx.x; q < p.count; q += gridDim.x) {
    const uint32_t ta = uniform32(p.a[q]), tb = uniform32(p.b[q]);
    const bool live = (ta == pd::kNone || uniform32(t.ok[ta]) != 0) && (tb == pd::kNone || uniform32(t.ok[tb]) != 0);
    Side A = side_of(t, buf, ta), B = side_of(t, buf, tb);
    if (!live) A.n = B.n = 0;
    uint32_t recs = 0;
    uint64_t bytes = 0;
    walk_side<kWrite, false>(A, B, p, q, lane, recs, bytes);
    walk_side<kWrite, true>(B, A, p, q, lane, recs, bytes);
    if (!kWrite && lane == 0) p.nrec[q] = recs, p.nbytes[q] = bytes;
  }
}

}  // namespace pkd
}  // namespace md

using namespace md::pkd;
constexpr uint32_t kMaxWaveGrid = 1u << 20;  // wavefronts of a launch that strides over its work

extern "C" int md_launch_pkd_tree_table(const md::pkd::Trees *t, const uint8_t *buf, hipStream_t stream) {
  if (t->count == 0) return 0;
  hipLaunchKernelGGL(tree_table_kernel, dim3(t->count < kMaxWaveGrid ? t->count : kMaxWaveGrid), dim3(kWave), 0, stream, *t, buf);
  return (int)hipGetLastError();
}
extern "C" int md_launch_pkd_tree_diff(const md::pkd::Trees *t, const md::pkd::Pairs *p, const uint8_t *buf, int write, hipStream_t stream) {
  if (p->count == 0) return 0;
  const dim3 grid(p->count < kMaxWaveGrid ? p->count : kMaxWaveGrid);
  if (write) hipLaunchKernelGGL(tree_diff_kernel<true>, grid, dim3(kWave), 0, stream, *t, *p, buf);
  else hipLaunchKernelGGL(tree_diff_kernel<false>, grid, dim3(kWave), 0, stream, *t, *p, buf);
  return (int)hipGetLastError();
}
