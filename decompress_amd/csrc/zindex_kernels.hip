// zindex_kernels.hip — the index of a long stream on the device (md_inflate_index_build, md_inflate_index_read;
// mdeflate.h), for gfx950.  The inflate kernel itself is the batch's (md_inflate_continue_batch_device); what is here
// surrounds it.
//
//   windows_take_kernel  build: one workgroup per (point, 4 KiB slice) copies the window in front of a new point out of the
//                        piece's decoded output (unaligned 16-byte loads, aligned 16-byte stores)
//   plan_kernel          read, one workgroup: marks in a bitmap the pieces that any range touches (a binary search over
//                        the points' output offsets per range end), then goes over the pieces from `first` on, 1 024 at a
//                        time: a prefix sum over the marked ones gives each its stream number, its place in the input blob
//                        and its slot; the pieces that fit the budget get their descriptors
//   windows_put_kernel   read: one workgroup per (piece, 4 KiB slice) writes the piece's window in front of its slot
//   verdict_kernel       read: one thread per piece: did its last complete block end exactly on the next point
//   gather_kernel        read: one wavefront per (range, 16 KiB segment) copies the bytes of the round's good pieces into
//                        the range (16-byte stores on the destination's alignment), and the range's status
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "mdeflate.h"

namespace md {
namespace zix {

constexpr uint32_t kWave = 64, kPlanThreads = 1024, kSlice = 4096, kSlices = (uint32_t)(kWin / kSlice);

__global__ __launch_bounds__(256) void windows_take_kernel(uint32_t n, const uint8_t *__restrict__ out, const uint64_t *__restrict__ src_off,
                                                           const uint32_t *__restrict__ wlen, uint8_t *__restrict__ wins) {
  const uint32_t p = blockIdx.y, at = blockIdx.x * kSlice + threadIdx.x * 16;
  if (p >= n) return;
  const uint32_t w = wlen[p];
  if (at >= w) return;
  const uint8_t *a = out + src_off[p] + at;
  uint8_t *o = wins + (uint64_t)p * kWin + at;
  if (at + 16 <= w) {
    uint4 v;
    __builtin_memcpy(&v, a, 16);
    *reinterpret_cast<uint4 *>(o) = v;
  } else {
    for (uint32_t i = 0; at + i < w; i++) o[i] = a[i];
  }
}

__global__ __launch_bounds__(256) void windows_put_kernel(uint32_t count, const uint8_t *__restrict__ wins, Round r, uint8_t *__restrict__ slots) {
  const uint32_t j = blockIdx.y, at = blockIdx.x * kSlice + threadIdx.x * 16;
  if (j >= count) return;
  const uint32_t w = r.hist_len[j];
  if (at >= w) return;
  const uint8_t *a = wins + (uint64_t)j * kWin + at;  // (both sides on 16 bytes: slots begin on 64)
  uint8_t *o = slots + r.out_off[j] + at;
  if (at + 16 <= w) *reinterpret_cast<uint4 *>(o) = *reinterpret_cast<const uint4 *>(a);
  else
    for (uint32_t i = 0; at + i < w; i++) o[i] = a[i];
}

// the piece that holds byte x of the output: the last point k with out[k] <= x (out[0] = 0; x < size)
__device__ __forceinline__ uint64_t piece_of(const uint64_t *__restrict__ out, uint64_t points, uint64_t x) {
  uint64_t lo = 0, hi = points;  // out[lo] <= x < out[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (out[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// inclusive prefix sums of one value per thread over the workgroup (v[] in LDS, kPlanThreads entries)
template <class T>
__device__ __forceinline__ T scan_inclusive(T *v, T mine, uint32_t tid) {
  v[tid] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < kPlanThreads; d <<= 1) {
    const T add = tid >= d ? v[tid - d] : 0;
    __syncthreads();
    v[tid] += add;
    __syncthreads();
  }
  return v[tid];
}

__global__ __launch_bounds__(kPlanThreads) void plan_kernel(Tables t, uint64_t n, const uint64_t *__restrict__ off, const uint64_t *__restrict__ len,
                                                            int mark, uint64_t first, uint64_t budget, uint32_t round, Round r,
                                                            uint64_t *__restrict__ plan) {
  __shared__ uint32_t s_cnt[kPlanThreads];
  __shared__ uint64_t s_slot[kPlanThreads], s_in[kPlanThreads];
  __shared__ unsigned long long s_stop;
  const uint32_t tid = threadIdx.x;
  const uint64_t P = t.points;
  if (mark) {
    for (uint64_t i = tid; i < n; i += kPlanThreads) {
      if (len[i] == 0) continue;
      const uint64_t a = piece_of(t.out, P, off[i]), b = piece_of(t.out, P, off[i] + len[i] - 1);
      for (uint64_t w = a / 32; w <= b / 32; w++) {
        uint32_t bits = 0xffffffffu;
        if (w == a / 32) bits &= 0xffffffffu << (a % 32);
        if (w == b / 32) bits &= 0xffffffffu >> (31 - b % 32);
        atomicOr(&t.marked[w], bits);
      }
    }
    __threadfence();
    __syncthreads();
  }
  uint64_t c_cnt = 0, c_slot = 0, c_in = 0;  // what the chunks before this one took (the same on every thread)
  for (uint64_t base = first; base < P; base += kPlanThreads) {
    if (tid == 0) s_stop = ~0ull;
    const uint64_t k = base + tid;
    const bool m = k < P && ((t.marked[k / 32] >> (k % 32)) & 1u);
    uint64_t in_at = 0, in_len = 0, hist = 0, cap = 0;
    if (m) {
      const uint64_t o = t.out[k];
      in_at = t.bit[k] >> 3;
      in_len = (k + 1 < P ? (t.bit[k + 1] + 7) >> 3 : t.body_end) - in_at;
      hist = o < kWin ? o : kWin;
      cap = hist + (k + 1 < P ? t.out[k + 1] : t.size) - o;
    }
    const uint32_t i_cnt = scan_inclusive<uint32_t>(s_cnt, m ? 1u : 0u, tid);
    const uint64_t i_slot = scan_inclusive<uint64_t>(s_slot, m ? slot_stride(cap) : 0, tid);
    const uint64_t i_in = scan_inclusive<uint64_t>(s_in, m ? in_stride(in_len) : 0, tid);
    const uint64_t j = c_cnt + i_cnt - (m ? 1 : 0), slot_at = c_slot + i_slot - (m ? slot_stride(cap) : 0),
                   blob_at = c_in + i_in - (m ? in_stride(in_len) : 0);
    // the slots are laid end to end, so the pieces that fit are a prefix of the marked ones; the first always goes
    if (m && j != 0 && c_slot + i_slot > budget) atomicMin(&s_stop, (unsigned long long)k);
    __syncthreads();
    const uint64_t stop = s_stop;
    if (m && k < stop) {
      r.in_off[j] = blob_at;
      r.in_len[j] = in_len;
      r.out_off[j] = slot_at;
      r.out_cap[j] = cap;
      r.start_bit[j] = (uint32_t)(t.bit[k] & 7);
      r.hist_len[j] = (uint32_t)hist;
      r.adler_in[j] = 1;
      r.piece[j] = (uint32_t)k;
      t.round_of[k] = round;
      t.place[k] = slot_at + hist;
    }
    if (stop != ~0ull) {
      if (k == stop) {  // (marked: what lies in front of it is the round)
        plan[kPlanCount] = j;
        plan[kPlanScratch] = slot_at;
        plan[kPlanIn] = blob_at;
        plan[kPlanNext] = stop;
      }
      return;
    }
    c_cnt += s_cnt[kPlanThreads - 1];
    c_slot += s_slot[kPlanThreads - 1];
    c_in += s_in[kPlanThreads - 1];
    __syncthreads();
  }
  if (tid == 0) {
    plan[kPlanCount] = c_cnt;
    plan[kPlanScratch] = c_slot;
    plan[kPlanIn] = c_in;
    plan[kPlanNext] = P;
  }
}

// A piece is good only if its last complete block ended exactly on the next point - bit and output offset -, or, for the
// last piece, the final block ended with exactly the output that is left: the rule of the long-stream decoder for its
// pieces (capi_long_stream.cpp).  Otherwise its ranges get the decoder's status, or MD_INVALID_INDEX where that says
// nothing wrong.
__global__ void verdict_kernel(uint32_t count, Tables t, Round r) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const uint64_t k = r.piece[j], hist = r.hist_len[j];
  const int32_t st = r.status[j];
  int32_t v;
  if (k + 1 < t.points) {
    const bool good = st == MD_UNEXPECTED_END_OF_INPUT && r.resume_last[j] == 0 && (t.bit[k] & ~(uint64_t)7) + r.resume_bits[j] == t.bit[k + 1] &&
                      r.resume_out[j] == hist + (t.out[k + 1] - t.out[k]);
    v = good ? MD_OK : st == MD_OK || st == MD_UNEXPECTED_END_OF_INPUT ? MD_INVALID_INDEX : st;
  } else {
    const bool good = st == MD_OK && r.out_len[j] == hist + (t.size - t.out[k]);
    v = good ? MD_OK : st == MD_OK ? MD_INVALID_INDEX : st;
  }
  t.verdict[k] = v;
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

// grid (ranges, segments): wavefront (i, y) copies segments y, y + gridDim.y, .. of range i; (i, 0) also looks at the
// verdicts of the range's pieces of this round.  Rounds go through the pieces in order, so the first verdict that is
// not MD_OK to reach status[i] is the first failing piece's.
__global__ __launch_bounds__(kWave) void gather_kernel(Tables t, uint64_t n, const uint64_t *__restrict__ off, const uint64_t *__restrict__ len,
                                                       uint32_t round, const uint8_t *__restrict__ slots, uint8_t *__restrict__ dst,
                                                       const uint64_t *__restrict__ dst_off, int32_t *__restrict__ status) {
  const uint64_t i = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  if (i >= n) return;
  const uint64_t L = len[i], o = off[i], P = t.points;
  if (L == 0) return;
  if (blockIdx.y == 0) {
    const uint64_t a = piece_of(t.out, P, o), b = piece_of(t.out, P, o + L - 1);
    unsigned long long bad = ~0ull;
    for (uint64_t k = a + lane; k <= b; k += kWave)
      if (t.round_of[k] == round && t.verdict[k] != MD_OK && k < bad) bad = k;
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long other = __shfl_xor(bad, d);
      bad = other < bad ? other : bad;
    }
    if (lane == 0 && bad != ~0ull) atomicCAS(&status[i], MD_OK, t.verdict[bad]);
  }
  const uint64_t nseg = (L + kGatherSegment - 1) / kGatherSegment;
  for (uint64_t s = blockIdx.y; s < nseg; s += gridDim.y) {
    uint64_t pos = o + s * kGatherSegment;
    const uint64_t end = o + L - pos < kGatherSegment ? o + L : pos + kGatherSegment;
    for (uint64_t k = piece_of(t.out, P, pos); pos < end; k++) {
      const uint64_t piece_end = k + 1 < P ? t.out[k + 1] : t.size, e = piece_end < end ? piece_end : end;
      if (t.round_of[k] == round && t.verdict[k] == MD_OK)
        wave_copy(dst + dst_off[i] + (pos - o), slots + t.place[k] + (pos - t.out[k]), e - pos, lane);
      pos = e;
    }
  }
}

}  // namespace zix
}  // namespace md

extern "C" int md_launch_zix_windows_take(uint32_t n, const uint8_t *out, const uint64_t *src_off, const uint32_t *wlen, uint8_t *wins,
                                          hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(md::zix::windows_take_kernel, dim3(md::zix::kSlices, n), dim3(256), 0, stream, n, out, src_off, wlen, wins);
  return (int)hipGetLastError();
}
extern "C" int md_launch_zix_plan(const md::zix::Tables *t, uint64_t n, const uint64_t *off, const uint64_t *len, int mark, uint64_t first,
                                  uint64_t budget, uint32_t round, const md::zix::Round *r, uint64_t *plan, hipStream_t stream) {
  hipLaunchKernelGGL(md::zix::plan_kernel, dim3(1), dim3(md::zix::kPlanThreads), 0, stream, *t, n, off, len, mark, first, budget, round, *r, plan);
  return (int)hipGetLastError();
}
extern "C" int md_launch_zix_windows_put(uint32_t count, const uint8_t *wins, const md::zix::Round *r, uint8_t *slots, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(md::zix::windows_put_kernel, dim3(md::zix::kSlices, count), dim3(256), 0, stream, count, wins, *r, slots);
  return (int)hipGetLastError();
}
extern "C" int md_launch_zix_verdict(uint32_t count, const md::zix::Tables *t, const md::zix::Round *r, hipStream_t stream) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(md::zix::verdict_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, count, *t, *r);
  return (int)hipGetLastError();
}
extern "C" int md_launch_zix_gather(const md::zix::Tables *t, uint64_t n, uint64_t longest, const uint64_t *off, const uint64_t *len,
                                    uint32_t round, const uint8_t *slots, uint8_t *dst, const uint64_t *dst_off, int32_t *status,
                                    hipStream_t stream) {
  if (n == 0 || longest == 0) return 0;
  const uint64_t nseg = (longest + md::zix::kGatherSegment - 1) / md::zix::kGatherSegment;
  hipLaunchKernelGGL(md::zix::gather_kernel, dim3((uint32_t)n, (uint32_t)(nseg < 4096 ? nseg : 4096)), dim3(md::zix::kWave), 0, stream, *t, n,
                     off, len, round, slots, dst, dst_off, status);
  return (int)hipGetLastError();
}
