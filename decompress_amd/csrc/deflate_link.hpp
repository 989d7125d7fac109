// deflate_link.hpp — the hash-chain insertion of deflate_link_kernel (deflate_front.hip) as a device function, shared with
// the segmented form for one long stream (deflate_chunked.hip).
//
// A workgroup of LW wavefronts inserts positions [lo, hi) of one stream into its 32 K-entry head table in LDS, in stream
// order, and writes link[p] for the positions p >= wlo of that range.  link[p] only depends on the positions of the
// previous 32 767 with the hash of p (what lies further back is written as 0), so a range that begins 32 KiB in front of
// wlo gives the same link[] on [wlo, hi) as one pass over the whole stream.  The head table afterwards holds, for every
// hash, the latest position of [lo, hi) with that hash.
#pragma once
#include "deflate_common.hpp"

namespace md {
namespace defl {

constexpr int PGL = 8;  // steps of 64 positions whose LDS atomics are in flight together (link kernel)
constexpr int LW = 16;  // wavefronts per stream

// the 4 bytes at pos (little-endian) for pos < p_end (something for the others), without a branch: Lz's last string (pos = len - 3) has
// only 3 bytes — it is taken from the word one byte earlier; len >= 4 whenever p_end > 1
__device__ __forceinline__ uint32_t load_w4(const uint8_t *__restrict__ src, uint32_t slen, uint32_t p_end, uint32_t pos) {
  uint32_t a = pos + 4 <= slen ? pos : slen - 4;
  a = pos < p_end ? a : 0u;
  uint32_t v;
  __builtin_memcpy(&v, src + a, 4);
  return v >> ((8 * (pos - a)) & 31);  // (whatever for pos >= p_end: nobody looks at it)
}

// head[h] <- max(pos), one LDS atomic per position.  The head table of a stream is 128 KiB of LDS, so a CU holds one
// stream — and one wavefront alone runs at the latency of its own instruction stream (9 cycles per instruction
// measured).  LW wavefronts therefore share the stream: wavefront w takes the groups k = w, w + LW, ... of 8 x 64
// positions, loads and hashes them ahead, and only the atomics themselves are taken in stream order — a turn counter
// in LDS lets group k issue its eight atomics once group k - 1 has got its results back (a wavefront's own LDS
// operations execute in order).  Everything after the atomics (sorting out equal hashes, the stores) overlaps with
// the other wavefronts' groups.  Measured per GiB of input: 4 wavefronts 4.9 ms (word text 7.0), 8: 3.1 (4.5), 16:
// 3.2 (3.8) — from 8 on the chain of turns is what is left.
// The values a set of equal hashes gets back are >= the head before the set and one of them is exactly that value: a
// lane that shares its hash with another lane of its step is recognised by a returned position inside the step, and
// such steps sort themselves out by ballots (the predecessor of a lane is the nearest lower lane with its hash, else
// the smallest value the set got back).
// NS = De.Def.Ns's hc_matchfinder (lib/de.ml:3765-3856): the hash is 16 bits of 4 bytes times 0x1E35A7BD — twice the
// table LDS has room for, so the stream is gone through twice, once per half of the hash range (a chain never leaves
// its half) —, position 0 goes into bucket 0 whatever its bytes (next_hash4 starts at 0), and there is no tail.
// Every thread of the workgroup calls this with the same arguments (it contains workgroup barriers).
template <bool NS>
__device__ __forceinline__ void link_insert(uint32_t *head, uint32_t *gmin, uint32_t *turn, const uint8_t *__restrict__ src,
                                            uint32_t slen, uint32_t p_end, uint32_t lo, uint32_t wlo, uint32_t hi,
                                            uint32_t *__restrict__ lk, int matcher, uint32_t pass) {
  // De.Lz77: position 0 is NIL (it can never be a match source there); Def.Ns: position 0 is an ordinary candidate, so
  // the table holds position + 1
  constexpr uint32_t bias = NS ? 1u : 0u;
  const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  __syncthreads();
  {
    uint4 *h4 = reinterpret_cast<uint4 *>(head);
    for (uint32_t i = threadIdx.x; i < (uint32_t)HASH_SIZE / 4; i += LW * kWave) h4[i] = make_uint4(0, 0, 0, 0);
    if (threadIdx.x == 0) *turn = 0;
  }
  __syncthreads();
  // the input of a wavefront's next two groups is requested before the current one is worked on
  // (branch-free: a branch around a load makes the compiler wait for every load in flight)
  auto load_group = [&](uint32_t pe, uint32_t (&w)[PGL]) {
#pragma unroll
    for (int g = 0; g < PGL; g++) w[g] = load_w4(src, slen, p_end, pe + g * kWave + lane);
  };
  constexpr uint32_t kGroup = PGL * kWave;
  const uint32_t ngroups = (hi - lo + kGroup - 1) / kGroup;
  uint32_t wa[PGL], wb[PGL];
  load_group(lo + wv * kGroup, wa);
  load_group(lo + (wv + LW) * kGroup, wb);
  for (uint32_t k = wv; k < ngroups; k += LW) {
    const uint32_t pe = lo + k * kGroup;
    uint32_t w4[PGL], hv[PGL], ret[PGL];
    bool mine[PGL];  // the position's hash is in this pass's half of the range
#pragma unroll
    for (int g = 0; g < PGL; g++) {
      w4[g] = wa[g];
      wa[g] = wb[g];
      if (NS) {
        const uint32_t h = (pe + g * kWave + lane) == 0 ? 0u : (uint32_t)(w4[g] * 0x1E35A7BDu) >> 16;
        hv[g] = h & (HASH_SIZE - 1);
        mine[g] = (h >> HASH_BITS) == pass;
      } else {
        hv[g] = hash_of(matcher, w4[g]);
        mine[g] = true;
      }
    }
    load_group(pe + 2 * LW * kGroup, wb);
    while (__hip_atomic_load(turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != k) __builtin_amdgcn_s_sleep(1);
#pragma unroll
    for (int g = 0; g < PGL; g++) {
      const uint32_t pos = pe + g * kWave + lane;
      ret[g] = (pos < hi && mine[g]) ? atomicMax(&head[hv[g]], pos + bias) : 0xffffffffu;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the group's atomics have been performed: the next group may go
    if (lane == 0) __hip_atomic_store(turn, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
    for (int g = 0; g < PGL; g++) {
      const uint32_t s0 = pe + g * kWave;
      if (s0 >= hi) break;  // uniform
      const uint32_t pos = s0 + lane;
      const bool valid = pos < hi && mine[g];
      uint32_t c1;
      if (__ballot(valid && ret[g] >= s0 + bias) == 0) {
        c1 = valid ? ret[g] : 0;  // no two lanes share a hash: every returned value is the head before the step
      } else {
        const uint32_t h = hv[g];
        uint64_t same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < HASH_BITS; bit++) {
          const bool mine = (h >> bit) & 1;
          const uint64_t bal = __ballot(mine);
          same &= mine ? bal : ~bal;
        }
        const uint64_t below = same & lanes_below(lane);
        const uint32_t first = valid ? (uint32_t)__builtin_ctzll(same) : lane;
        gmin[lane] = 0xffffffffu;
        __builtin_amdgcn_wave_barrier();
        if (valid) atomicMin(&gmin[first], ret[g]);
        __builtin_amdgcn_wave_barrier();
        c1 = !valid ? 0u : below ? s0 + bias + 63u - (uint32_t)__builtin_clzll(below) : __hip_atomic_load(&gmin[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_wave_barrier();
      }
      if (valid && pos >= wlo) {
        const uint32_t d = pos + bias - c1;
        lk[pos] = ((c1 != 0 && d <= 32767u) ? d : 0u) | (fp16(w4[g]) << 16);
      }
    }
  }
}

// De's position len - 3 (lookahead 3): hash4 reads a 4th byte beyond the data (H7) — zero before the first slide of
// the reference's 64 KiB buffer, the byte 32 KiB earlier after it.  Which one depends on the matcher's trajectory:
// both heads are handed over.  Threads 0 and 1 of the workgroup, after the last insertion and a barrier; the table
// must hold every position of the last 32 KiB before len - 3 (a head further back is never a candidate: the matcher
// only takes one within MAX_DIST, and 0 is as good as one beyond).
__device__ __forceinline__ void link_tail(const uint32_t *head, const uint8_t *__restrict__ src, uint32_t slen, int matcher,
                                          uint32_t *__restrict__ tail2) {
  if (threadIdx.x < 2) {
    uint32_t res = 0;
    if (matcher == MD_MATCHER_DE && slen >= 3) {
      const uint32_t p = slen - 3;
      const uint32_t b3 = (threadIdx.x == 1 && slen >= (uint32_t)WSIZE) ? src[slen - WSIZE] : 0u;
      const uint32_t w = (uint32_t)src[p] | ((uint32_t)src[p + 1] << 8) | ((uint32_t)src[p + 2] << 16) | (b3 << 24);
      res = head[hash_of(matcher, w)];
    }
    tail2[threadIdx.x] = res;
  }
}

}  // namespace defl
}  // namespace md
