// inflate_wave.hip — batched RFC1951 inflate for gfx950 (MI355X): one kernel, one workgroup of two wavefronts per stream.
//
// The DECODER wavefront finds and decodes tokens (sync, emit below); the COPIER wavefront resolves the matches and
// writes the round out (copy, flush).  They share the stream's LDS (staging buffer, match records) and hand rounds
// over through a mailbox in LDS (struct Mail): while the copier works on round r the decoder is already walking the
// zones of round r + 1, and it waits for the copier only before it writes round r + 1 into the staging buffer.  One
// stream's rounds are serial, its two halves are not: a stream finishes 1.4x sooner than with one wavefront doing both
// in turn (that form is still here: md_set_option "inflate_waves" = 1, same results), and with 8 streams = 16
// wavefronts per CU the kernel is 1.13x faster on C2.  Since round 7 a stream's LDS (17 872 B) and the PAIR form's
// VGPRs (<= 96) leave room for 9 streams = 18 wavefronts per CU: 2.6 % faster on C2.
//
// The decoder's 64 lanes decode 64 consecutive zones (48 .. S bits, re-sized every round from what the last one produced) of
// the compressed block per round:
//
//   sync   Light passes that only FIND TOKEN BOUNDARIES.  Pass 0: lane i walks the tokens from bit
//          bp + i*S until it crosses bp + (i+1)*S (only lane 0 starts on a boundary, the others
//          are speculative).  Pass k >= 1: a lane whose left neighbour ended somewhere else than
//          where it started walks again from there and now also counts the bytes and matches its
//          tokens will produce.  Huffman streams re-synchronise (p ~ 0.9 inside a full zone), so the
//          chain start_i == end_{i-1} settles after ~4 passes; the consistent prefix of lanes is
//          accepted.  A chain of token boundaries that starts on a known boundary IS the serial
//          decode of the reference loop (`inflate`, lib/de.ml:1667-1712).  A walk step is one
//          32-bit peek of the input window in LDS and one 32-bit LUT entry that carries the bits
//          to skip and the descriptor (index width, base) of the table the NEXT step indexes, so
//          the step has no per-type branches or selects.
//   emit   One pass over the accepted lanes from their validated starts.  A wave prefix sum of
//          the counts has given every lane its output position and its first record, so literals
//          go straight to their final place in the LDS staging buffer and matches become (length,
//          distance, position) records in one pool, in stream order.  Anything unusual (end of
//          block, an invalid code, a distance or length the output cannot take, a full buffer)
//          stops the lane in front of the token; the token is then looked at again with the checks
//          in the reference's order.
//   copy   By record, 64 per step across the wave.  Matches whose source is older than the round
//          read it from already flushed output (L2/HBM, up to 32 bytes per record, all of the
//          round's records in flight together); matches into the round itself are listed and wait
//          on a bitmap of the staging bytes that are still to be produced; long and self-overlapping
//          ones are copied by the whole wave.
//   flush  16-byte coalesced stores, Adler-32 folded in the same pass with v_dot4_u32_u8
//          (WInf.update / tail, lib/de.ml:453-455, 499-505).
//
// The window is the output buffer itself (De.Inf.Ns semantics, lib/de.ml:1534).  Block headers
// (lib/de.ml:1733-1793) are parsed wave-uniform on the scalar unit; the Huffman tables
// (De.Inf.huffman, lib/de.ml:523-638) are built by all lanes from the canonical code.  Stored
// blocks (lib/de.ml:1613-1627) and the zlib frame (lib/zl.ml:400-417) run between rounds.  The first
// failing token in stream order decides the status and everything before it is written
// (oracle/de_inflate.c).
// Record pool and staging buffer: together with the table and the window they decide how many streams a CU holds.
// 576 records are nine far rows (copy_far), which keeps the PAIR form at <= 96 VGPRs without scratch (five wavefronts per
// SIMD); with 5248 staging bytes a stream needs 17 872 B of LDS, 9 streams per CU.  Measured on C2 (ms): 768 / 5568 at 8
// streams 4.24; 576 / 5248 at 9 streams 4.11; 576 / 5568 (18 192 B, still 8: the LDS is allocated in coarser units)
// 4.29; 576 / 3760 at 10 streams 4.78 (rounds too short).  -DMD_RMAX / -DMD_STAGE / -DMD_PAIR_OCC: measurement builds.
#ifndef MD_RMAX
#define MD_RMAX 576
#endif
#ifndef MD_STAGE
#define MD_STAGE 5248
#endif
#ifndef MD_PAIR_OCC
#define MD_PAIR_OCC 5  // wavefronts per SIMD the PAIR form is compiled for (launch bounds): 18 per CU need 5 on two SIMDs
#endif
#include "inflate_wave_core.hpp"

namespace md {
namespace wv {

// ---- output -------------------------------------------------------------------------------------
struct Sink {
  lds_u8 *stage;
  uint8_t *g;
  uint32_t cap;
  uint32_t pos;  // bytes produced and flushed
  uint32_t lane;
  uint32_t a, b;
  bool want_adler;
  __device__ __forceinline__ uint32_t sbase() const { return pos & ~15u; }  // staging index of position x is x - sbase()

  // write stage[...] for positions [pos, pos+total) to HBM, fold Adler-32, advance pos: whole 16-byte chunks one per
  // lane, the bytes of the (at most two) partial chunks at either end one per lane
  __device__ __forceinline__ void flush(uint32_t total) {
    const uint32_t rb = sbase();
    const uint32_t endp = pos + total;
    const uint32_t full0 = (pos + 15) & ~15u, full1 = endp & ~15u;  // whole chunks: [full0, full1) (if full0 < full1)
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t ps = full0; ps < full1; ps += 1024) {
      const uint32_t cpos = ps + lane * 16;
      if (cpos < full1) {
        const lds_u32 *sp = reinterpret_cast<const lds_u32 *>(stage + (cpos - rb));  // 16-byte aligned
        const uint32_t w0 = sp[0], w1 = sp[1], w2 = sp[2], w3 = sp[3];
        const uint4 v = make_uint4(w0, w1, w2, w3);
        __builtin_memcpy(g + cpos, &v, 16);
        if (want_adler) {
          // sum d_k and sum k*d_k over the 16 bytes
          uint32_t t1 = __builtin_amdgcn_udot4(w0, 0x01010101u, 0u, false);
          t1 = __builtin_amdgcn_udot4(w1, 0x01010101u, t1, false);
          t1 = __builtin_amdgcn_udot4(w2, 0x01010101u, t1, false);
          t1 = __builtin_amdgcn_udot4(w3, 0x01010101u, t1, false);
          uint32_t tk = __builtin_amdgcn_udot4(w0, 0x03020100u, 0u, false);
          tk = __builtin_amdgcn_udot4(w1, 0x07060504u, tk, false);
          tk = __builtin_amdgcn_udot4(w2, 0x0b0a0908u, tk, false);
          tk = __builtin_amdgcn_udot4(w3, 0x0f0e0d0cu, tk, false);
          s1 += t1;
          s2 += (endp - cpos) * t1 - tk;
        }
      }
    }
    {  // lanes 0..15: the bytes in front of the first whole chunk; lanes 16..31: the bytes behind the last one
      const uint32_t head1 = full0 < endp ? full0 : endp;     // head: [pos, head1)
      const uint32_t tail0 = full1 > head1 ? full1 : head1;   // tail: [tail0, endp)
      const uint32_t x = lane < 16 ? pos + lane : tail0 + (lane - 16);
      if (lane < 16 ? x < head1 : (lane < 32 && x < endp)) {
        const uint32_t d = stage[x - rb];
        g[x] = (uint8_t)d;
        s1 += d;
        s2 += (endp - x) * d;
      }
    }
    if (want_adler) {  // per lane: <= 96 bytes x 255 x 6160 < 2^32
      s1 = wave_sum(s1);
      s2 = wave_sum(s2 % 65521u);
      b = (b + total * a + s2) % 65521u;
      a = (a + s1) % 65521u;
    }
    pos = endp;
  }
};

// ---- the measurement build ------------------------------------------------------------------------
// -DMD_DEBUG_KNOWN_BOUNDS only (tools/dbg/build_known_bounds.sh): mode & 3 == 1 records what the sync
// passes of every round found (start, end, stop, counts per lane), == 2 replays the record instead of walking - the
// time of that launch is what a PERFECT sync would leave of the kernel.  mode & 4: the copier skips the matches (far and
// near) and only flushes; mode & 8: the copier does nothing at all (the decoder's time alone).  Results are only right in
// modes 0..2.  The product build has the empty form: nothing of it is left in the kernel.
#ifdef MD_DEBUG_KNOWN_BOUNDS
constexpr uint32_t KB_ROUNDS = 512;
__device__ uint4 *g_kb_buf;
__device__ int g_kb_mode;
struct KnownBounds {
  uint32_t round, sid;
  uint4 *slot;  // of the round at hand, or null: beyond the record
  __device__ __forceinline__ void init(uint32_t stream) { round = 0, sid = stream; }
  // called once a round, in front of the sync passes: true = r is the replayed record, they are not walked
  __device__ __forceinline__ bool replay(SyncRound &r, uint32_t rbp, uint32_t zs, uint32_t lane) {
    slot = round < KB_ROUNDS ? g_kb_buf + ((size_t)sid * KB_ROUNDS + round) * kWave + lane : nullptr;
    round++;
    if ((__builtin_amdgcn_readfirstlane(g_kb_mode) & 3) != 2 || !slot) return false;
    const uint4 v = *slot;
    r.start = v.x, r.end = v.y, r.stop = v.z & 0xffffu, r.counted = (v.z >> 16) != 0, r.nb = v.w;
    r.limit = rbp + (lane + 1) * zs;
    r.midp = 0xffffffffu, r.midcnt = 0, r.np = 0;
    r.nvalid = consistent_prefix(r, lane);
    return true;
  }
  __device__ __forceinline__ void record(const SyncRound &r) {
    if ((__builtin_amdgcn_readfirstlane(g_kb_mode) & 3) == 1 && slot) *slot = make_uint4(r.start, r.end, r.stop | (r.counted ? 0x10000u : 0u), r.nb);
  }
  // the copier's ablations: true = the round has been dealt with
  static __device__ __forceinline__ bool skip_copy(Sink &sk, uint32_t total) {
    const int kbm = __builtin_amdgcn_readfirstlane(g_kb_mode);
    if (kbm & 8) sk.pos += total;
    else if (kbm & 4) sk.flush(total);
    return (kbm & 12) != 0;
  }
};
#else
struct KnownBounds {
  __device__ __forceinline__ void init(uint32_t) {}
  __device__ __forceinline__ bool replay(SyncRound &, uint32_t, uint32_t, uint32_t) { return false; }
  __device__ __forceinline__ void record(const SyncRound &) {}
  static __device__ __forceinline__ bool skip_copy(Sink &, uint32_t) { return false; }
};
#endif

// Far matches (the whole source is older than this round: final in HBM/L2 once the flush of earlier rounds has
// been waited for; d >= ml) and the heads of matches that straddle the round start.  The round's records are taken
// in stream order, one per lane and row of 64.  FIRST the loads of ALL rows are started - 2 LDS reads per record, one
// unaligned 16-byte load each: the source lies in L2 or beyond, two microseconds away on a busy chip, and a round
// should wait for that once, not once per group of rows (three sets of four rows, two of them in flight, spent more
// time waiting than working) - and while they are in flight the near matches are listed,
// in stream order, for copy_near_all (*nnear_out of them).  THEN the rows are gone through again as their data
// arrives: the record is read once more (cheaper than keeping three more registers per row) and its bytes are stored
// with exact-length LDS stores; bytes 16 .. 31 of the longer records follow in a second batch of the same kind, and
// what is beyond 32 bytes is copied by the whole wave, 8 bytes per lane, four records at a time.
// The loads read whole 8-byte words, up to 15 bytes past a record's source: the caller makes sure that stays inside
// the output buffer.
constexpr int FR = RMAX / kWave;  // rows of a full record pool
struct FarRow {
  uint32_t qs, n, src;
  bool near, has;
  uint32_t ml;
};
__device__ __forceinline__ FarRow far_row(const lds_u32 *mrec, const lds_u16 *mpos, uint32_t r, uint32_t nrec, uint32_t rb, uint32_t R0) {
  FarRow f;
  f.has = r < nrec;
  const uint32_t tk = mrec[f.has ? r : 0u];
  f.qs = mpos[f.has ? r : 0u];
  f.ml = rec_len(tk);
  const uint32_t s = rb + f.qs - rec_dist(tk);
  f.near = f.has && (tk & kNearBit);
  const uint32_t head = s < R0 ? R0 - s : 0u;  // a near match that begins before the round start: its head is final too
  f.n = !f.has ? 0u : f.near ? head : f.ml;
  f.src = f.n ? s : 0u;  // (a lane without a record reads g[0..15]: no branch around the load)
  return f;
}
template <class PF>
__device__ __forceinline__ void copy_far(const lds_u32 *mrec, const lds_u16 *mpos, lds_u16 *list, const Sink &sk,
                                         uint32_t lane, uint32_t nrec, uint32_t *nnear_out, PF &pf) {
  lds_u8 *stage = sk.stage;
  const uint32_t R0 = sk.pos, rb = sk.sbase();
  const uint8_t *g = sk.g;
  uint32_t nnear = 0;
  uint64_t v0[FR], v1[FR];
  // ONE pass over the records' rows: the loads of a row are started, the row's near matches and long records are listed
  // while they fly, and what the stores will need - staging position and byte count - stays in a register per row, so
  // that a record is read from LDS once, not three times (rounds 3-4: a pass to start the loads, one to list, one to store;
  // the same time within noise, seven registers fewer).  Straight-line: a load behind a branch makes the compiler wait
  // for it at the join; a row beyond the last record reads g[0..15] with every lane, one cache line
  uint32_t pk[FR];
  uint32_t nlong = 0;
  bool spill = false;
#pragma unroll
  for (int u = 0; u < FR; u++) {
    const FarRow f = far_row(mrec, mpos, u * kWave + lane, nrec, rb, R0);
    v0[u] = out_ld64(g + f.src);
    v1[u] = out_ld64(g + f.src + 8);
    pk[u] = f.qs | (f.n << 16);
    const uint64_t nb = __ballot(f.near);
    if (f.near) list[nnear + lane_rank(nb)] = (uint16_t)(u * kWave + lane);
    nnear += (uint32_t)__builtin_popcountll(nb);
    const uint64_t lb = __ballot(f.n > 16);
    const uint32_t lc = (uint32_t)__builtin_popcountll(lb);
    if (nnear + nlong + lc > RMAX) {  // the two lists would meet (a record can be in both): the long ones go the slow way
      spill = true;
      nlong = 0;
    }
    if (lb && !spill) {
      if (f.n > 16) list[RMAX - 1 - (nlong + lane_rank(lb))] = (uint16_t)(u * kWave + lane);
      nlong += lc;
    }
  }
  pf.tick_lds(P_FAR_REC);
#pragma unroll
  for (int u = 0; u < FR; u++) {
    if ((uint32_t)u * kWave < nrec) {
      const uint32_t qs = pk[u] & 0xffffu, n = pk[u] >> 16;
      if constexpr (PF::on) {
        if (u == 0) {
          asm volatile("" ::"v"(v0[u]), "v"(v1[u]));
          pf.tick_all(P_FAR_LOAD);
        }
      }
      if (n) {
        lds_u8 *dd = stage + qs;
        lds_put(dd, v0[u], n < 8 ? n : 8);
        if (n > 8) lds_put(dd + 8, v1[u], n < 16 ? n - 8 : 8);
      }
    }
  }
  pf.tick_lds(P_FAR);
  // bytes 16 .. 31 of the long ones: one record per lane again, all loads first
  for (uint32_t c0 = 0; c0 < nlong; c0 += kWave) {
    const bool has = c0 + lane < nlong;
    const uint32_t r = has ? list[RMAX - 1 - (c0 + lane)] : 0u;
    const FarRow f = far_row(mrec, mpos, r, nrec, rb, R0);
    const uint32_t n = has ? f.n : 0u;  // > 16 where there is a record
    const uint64_t w0 = out_ld64(g + (n ? f.src + 16 : 0u)), w1 = out_ld64(g + (n ? f.src + 24 : 0u));
    if (n) {
      lds_u8 *dd = stage + f.qs + 16;
      lds_put(dd, w0, n < 24 ? n - 16 : 8);
      if (n > 24) lds_put(dd + 8, w1, n < 32 ? n - 24 : 8);
    }
    // what is beyond 32 bytes: by the whole wave, 8 bytes per lane, four records' loads in flight at a time
    for (uint64_t lm = __ballot(n > 32); lm;) {
      uint32_t ln[4], lsrc[4], lqs[4];
      uint64_t d[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool any = lm != 0;
        const uint32_t l = any ? (uint32_t)__builtin_ctzll(lm) : 0u;
        lm &= lm - 1;  // (0 stays 0)
        ln[k] = any ? rdlane(n, l) : 0u;
        lsrc[k] = rdlane(f.src, l);
        lqs[k] = rdlane(f.qs, l);
      }
      const uint32_t j = 32 + lane * 8;
#pragma unroll
      for (int k = 0; k < 4; k++) d[k] = out_ld64(g + (j < ln[k] ? lsrc[k] + j : 0u));
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (j < ln[k]) lds_put(stage + lqs[k] + j, d[k], ln[k] - j < 8 ? ln[k] - j : 8);
    }
  }
  if (spill) {  // (rare: more long records than `list` has room for) one record at a time, all its bytes beyond 16
    pf.count(C_FAR_SPILL);
    for (uint32_t c0 = 0; c0 < nrec; c0 += kWave) {
      const FarRow f = far_row(mrec, mpos, c0 + lane, nrec, rb, R0);
      for (uint64_t lm = __ballot(f.n > 16); lm; lm &= lm - 1) {
        const uint32_t l = (uint32_t)__builtin_ctzll(lm);
        const uint32_t ln = rdlane(f.n, l), lsrc = rdlane(f.src, l), lqs = rdlane(f.qs, l);
        const uint32_t j = 16 + lane * 8;
        if (j < ln) lds_put(stage + lqs + j, out_ld64(g + lsrc + j), ln - j < 8 ? ln - j : 8);
      }
    }
  }
  pf.tick_all(P_FAR);
  *nnear_out = nnear;
}
// the same for the last rounds of a stream, where an 8-byte load could reach past the output buffer: guarded loads
template <class PF>
__device__ __noinline__ void copy_far_guarded(const lds_u32 *mrec, const lds_u16 *mpos, lds_u16 *list,
                                              lds_u8 *stage, const uint8_t *g, uint32_t R0, uint32_t rb, uint32_t cap,
                                              uint32_t lane, uint32_t nrec, uint32_t *nnear_out) {
  uint32_t nnear = 0;
  for (uint32_t c0 = 0; c0 < nrec; c0 += kWave) {
    const uint32_t r = c0 + lane;
    const FarRow f = far_row(mrec, mpos, r, nrec, rb, R0);
    const uint64_t nb = __ballot(f.near);
    if (f.near) list[nnear + lane_rank(nb)] = (uint16_t)r;
    nnear += (uint32_t)__builtin_popcountll(nb);
    for (uint32_t j = 0; j < f.n; j += 8) lds_put(stage + f.qs + j, out_ld_guard(g, f.src + j, f.n - j, cap), f.n - j < 8 ? f.n - j : 8);
  }
  *nnear_out = nnear;
}

// staging -> staging LZ77 copy of n bytes with forward-byte semantics (dst - src = d; overlap allowed), by the whole
// wave: one long or self-overlapping match at a time (dd, ss, n, d are wave-uniform).  Every destination byte j is
// stage[ss + j mod d], and the first period [ss, ss + min(d, n)) is final when the match is ready, so the lanes are
// independent of each other: 8 bytes per lane without overlap, one whole number of periods per lane for d < 8, 4
// gathered bytes per lane otherwise.
__device__ __forceinline__ void wave_copy(lds_u8 *stage, uint32_t dd, uint32_t ss, uint32_t n, uint32_t d, uint32_t lane) {
  if (d >= n) {
    const uint32_t j = lane * 8;
    if (j < n) lds_put(stage + dd + j, lds_ld64(stage + ss + j), n - j < 8 ? n - j : 8);
  } else if (d < 8) {
    uint64_t v = lds_ld64(stage + ss);  // the same 8 bytes for every lane
    const uint32_t sh = 8 * d;
    v &= (1ull << sh) - 1;
    v |= v << sh;
    if (2 * sh < 64) v |= v << (2 * sh);
    if (4 * sh < 64) v |= v << (4 * sh);
    const uint32_t adv = (0x76586880u >> (4 * d)) & 15;  // d * (8 / d): 5..8 bytes, 64 lanes cover 258
    const uint32_t j = lane * adv;
    if (j < n) lds_put(stage + dd + j, v, n - j < adv ? n - j : adv);
  } else {
    const float inv = 1.0f / (float)d;
    for (uint32_t j = lane * 4; j < n; j += 4 * kWave) {
      uint32_t r = j - (uint32_t)((float)j * inv) * d;  // j mod d, the quotient may be one off either way
      r = (int32_t)r < 0 ? r + d : r;
      r = r >= d ? r - d : r;
      uint32_t w = 0;
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) {
        const uint32_t x = r + k >= d ? r + k - d : r + k;  // d >= 8: one wrap at most
        w |= (uint32_t)stage[ss + x] << (8 * k);
      }
      lds_put(stage + dd + j, w, n - j < 4 ? n - j : 4);
    }
  }
}

// Near matches: the source reaches into this round's staging buffer.  copy_far listed them in stream order; they
// are taken 64 at a time, one per lane, whatever lane decoded them.  Everything a record of a group can depend on is
// an earlier group (done) or the group itself.  Inside a group the records' destinations are disjoint and ascending
// with the lane, so the records whose output a lane's source range [sa, sb) touches are a RANGE of lower lanes: found
// once per group by two binary searches over the lanes (ds_bpermute), kept as a 64-bit mask.  A record is copied in the
// pass in which all of them are done (a wave-uniform mask of finished lanes); the lowest lane left never waits, so every
// pass makes progress.  (Until round 5 this was a bitmap of pending staging bytes in LDS: two atomics to set, two loads
// to test and two atomics to clear per record and pass.)
template <class PF>
__device__ __forceinline__ void copy_near_all(const lds_u32 *mrec, const lds_u16 *mpos, const lds_u16 *list,
                                              const Sink &sk, uint32_t lane, uint32_t count, bool *stuck, PF &pf) {
  lds_u8 *stage = sk.stage;
  const uint32_t head = sk.pos - sk.sbase();  // staging index of the round start
  for (uint32_t c0 = 0; c0 < count; c0 += kWave) {
    bool todo = c0 + lane < count;
    const uint32_t e = todo ? list[c0 + lane] : 0u;
    const uint32_t tk = mrec[e], qs = mpos[e];
    const uint32_t d = rec_dist(tk), ml = rec_len(tk);
    // source bytes: staging [qs - d, min(qs - d + ml, qs)); the part before the round start came from HBM (copy_far)
    const int32_t s0 = (int32_t)qs - (int32_t)d;
    const uint32_t skip = s0 < (int32_t)head ? head - (uint32_t)s0 : 0u;
    const uint32_t sa = (uint32_t)(s0 + (int32_t)skip), sb = d < ml ? qs : (uint32_t)s0 + ml;
    const uint32_t n = ml - skip;         // skip < ml: a near match reaches into the round
    const bool fast = d >= n && n <= 32;  // the usual case: source and destination do not overlap
    // what the lanes of this group still have to produce: [qb, qe), ascending with the lane (idle lanes: nothing, on top)
    const uint32_t qb = todo ? qs + skip : 0xffffffffu, qe = todo ? qs + ml : 0xffffffffu;
    uint32_t jlo = 0, jhi = 0;  // lanes [jlo, jhi): qe > sa and qb < sb
#pragma unroll
    for (uint32_t st = 32; st > 0; st >>= 1) {
      const uint32_t ve = __shfl(qe, jlo + st - 1), vb = __shfl(qb, jhi + st - 1);
      jlo = ve <= sa ? jlo + st : jlo;
      jhi = vb < sb ? jhi + st : jhi;
    }
    jhi = jhi < lane ? jhi : lane;  // (lower lanes only: a record's own output is not its source)
    uint64_t need = 0;
    if (sa < sb && jlo < jhi) need = ((jhi >= 64 ? 0ull : (1ull << jhi)) - 1ull) & ~((1ull << jlo) - 1ull);
    uint64_t done = 0;  // wave-uniform: lanes of this group that are copied
    pf.tick_lds(P_NEAR_LOAD);
    for (uint32_t guard = 0; __ballot(todo) != 0; guard++) {
      if (guard > kWave) {  // cannot happen
        *stuck = true;
        return;
      }
      pf.count(C_NEAR_IT);
      const bool ready = todo && (need & ~done) == 0;
      if constexpr (PF::on) {
        if (__ballot(ready && !fast)) pf.count(C_LONG_NEAR);
      }
      pf.tick_lds(P_NEAR);
      if (ready && fast) {  // all loads in flight together
        lds_u8 *dd = stage + qs + skip;
        const lds_u8 *ss = stage + sa;
        const uint64_t v0 = lds_ld64(ss), v1 = lds_ld64(ss + 8), v2 = lds_ld64(ss + 16), v3 = lds_ld64(ss + 24);
        lds_put(dd, v0, n < 8 ? n : 8);
        if (n > 8) lds_put(dd + 8, v1, n < 16 ? n - 8 : 8);
        if (n > 16) {
          lds_put(dd + 16, v2, n < 24 ? n - 16 : 8);
          if (n > 24) lds_put(dd + 24, v3, n - 24);
        }
      }
      pf.tick_lds(P_NEAR_FAST);
      for (uint64_t lm = __ballot(ready && !fast); lm; lm &= lm - 1) {  // long or self-overlapping: the wave takes them one by one
        const uint32_t l = (uint32_t)__builtin_ctzll(lm);
        wave_copy(stage, rdlane(qs + skip, l), rdlane(sa, l), rdlane(n, l), rdlane(d, l), lane);
      }
      pf.tick_lds(P_NEAR_SLOW);
      done |= __ballot(ready);
      todo = todo && !ready;
      pf.tick_lds(P_NEAR_UPD);
    }
  }
  pf.tick(P_NEAR);
}

// The second half of a round: far matches from HBM, near matches inside the staging buffer, then the round goes out.
template <class PF>
__device__ __forceinline__ void copy_round(lds_smem *sm, Sink &sk, uint32_t lane, uint32_t total, uint32_t nrec, bool *stuck, PF &pf) {
  const lds_u32 *mrec = (const lds_u32 *)sm->mrec;
  const lds_u16 *mpos = (const lds_u16 *)sm->mpos;
  lds_u16 *list = (lds_u16 *)sm->list;
  const uint32_t R0 = sk.pos, rb = sk.sbase();
  uint32_t nnear = 0;
  if (KnownBounds::skip_copy(sk, total)) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // earlier rounds' flushes have landed
  if (R0 + 40 > sk.cap) {
    copy_far_guarded<PF>(mrec, mpos, list, sk.stage, sk.g, R0, rb, sk.cap, lane, nrec, &nnear);
    pf.tick(P_FAR);
  } else {
    copy_far(mrec, mpos, list, sk, lane, nrec, &nnear, pf);
  }
  copy_near_all(mrec, mpos, list, sk, lane, nnear, stuck, pf);
  sk.flush(total);
  pf.tick(P_ADLER);
}

// ---- the decoder / copier hand-over -------------------------------------------------------------
__device__ __forceinline__ uint32_t mail_ld(const MD_LDS uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void mail_st(MD_LDS uint32_t *p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// decoder: until the copier has finished everything posted so far (false = the copier gave up)
__device__ __forceinline__ bool mail_wait_idle(lds_smem *sm, uint32_t sent) {
  while (uni(mail_ld(&sm->mail.copied)) != sent) __builtin_amdgcn_s_sleep(2);  // (a poll costs issue slots the other wavefronts want)
  asm volatile("" ::: "memory");
  return uni(mail_ld(&sm->mail.stuck)) == 0;
}
// decoder: everything the job needs is in LDS; hand it over
__device__ __forceinline__ void mail_post(lds_smem *sm, uint32_t lane, uint32_t kind, uint32_t total, uint32_t x, uint32_t &sent) {
  if (lane == 0) {
    sm->mail.kind = kind;
    sm->mail.total = total;
    sm->mail.x = x;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  sent++;
  if (lane == 0) mail_st(&sm->mail.emitted, sent);
}

// kJobEmit (inflate_wave_core.hpp): the job lies in `list`, the copier's own array, idle between two rounds - every lane's
// request, behind them the wave-uniform words; the lanes' results come back in the words of their requests.
struct EmitHalf {  // the second half of a lane's zone
  uint32_t start, limit;  // window bits (start 0xffffffff: nothing to do)
  uint32_t q0, rec0;      // output position of its first byte, its first record
};
struct EmitUni {  // emit_pass's arguments that are the same for all lanes; checked: emit_pass<true>
  uint32_t lroot, tot, rb, R0, cap, checked;
};
struct EmitJob {
  union {
    EmitHalf ask;
    LaneOut got;
  } lane[kWave];
  EmitUni uni;
};
static_assert(offsetof(EmitJob, uni) == kHxUni * 4 && sizeof(EmitJob) == (kHxUni + 6) * 4, "the emit job's words in `list`");
__device__ __forceinline__ MD_LDS EmitJob *emit_job(lds_smem *sm) { return reinterpret_cast<MD_LDS EmitJob *>(sm->list); }
__device__ __forceinline__ void emit_ask(lds_smem *sm, uint32_t lane, const EmitHalf &h, const EmitUni &u) {
  MD_LDS EmitJob *j = emit_job(sm);
  j->lane[lane].ask.start = h.start, j->lane[lane].ask.limit = h.limit, j->lane[lane].ask.q0 = h.q0, j->lane[lane].ask.rec0 = h.rec0;
  if (lane == 0) j->uni.lroot = u.lroot, j->uni.tot = u.tot, j->uni.rb = u.rb, j->uni.R0 = u.R0, j->uni.cap = u.cap, j->uni.checked = u.checked;
}
__device__ __forceinline__ void emit_asked(lds_smem *sm, uint32_t lane, EmitHalf &h, EmitUni &u) {
  const MD_LDS EmitJob *j = emit_job(sm);
  h.start = j->lane[lane].ask.start, h.limit = j->lane[lane].ask.limit, h.q0 = j->lane[lane].ask.q0, h.rec0 = j->lane[lane].ask.rec0;
  u.lroot = uni(j->uni.lroot), u.tot = uni(j->uni.tot), u.rb = uni(j->uni.rb), u.R0 = uni(j->uni.R0), u.cap = uni(j->uni.cap);
  u.checked = uni(j->uni.checked);
}
__device__ __forceinline__ void emit_reply(lds_smem *sm, uint32_t lane, const LaneOut &lo) {
  MD_LDS EmitJob *j = emit_job(sm);
  j->lane[lane].got.endp = lo.endp, j->lane[lane].got.stopc = lo.stopc, j->lane[lane].got.bytes = lo.bytes, j->lane[lane].got.nm = lo.nm;
}
__device__ __forceinline__ LaneOut emit_replied(lds_smem *sm, uint32_t lane) {
  const MD_LDS EmitJob *j = emit_job(sm);
  LaneOut lo;
  lo.endp = j->lane[lane].got.endp, lo.stopc = j->lane[lane].got.stopc, lo.bytes = j->lane[lane].got.bytes, lo.nm = j->lane[lane].got.nm;
  return lo;
}
// a lane's verdict: its first half's if that stopped, else its second half's (bq, br: what the first half produces)
__device__ __forceinline__ LaneOut merge_halves(const LaneOut &a, const LaneOut &b, uint32_t bq, uint32_t br) {
  if (a.stopc != 0) return a;
  LaneOut lo;
  lo.endp = b.endp;
  lo.stopc = b.stopc;
  lo.bytes = bq + b.bytes;
  lo.nm = br + b.nm;
  return lo;
}

// ---- the phases of a round (inflate_block) ---------------------------------------------------------
// Staging and record capacity: of the consistent lanes, keep the largest prefix that fits (a lone first lane truncates
// itself; its matches always fit).  Every kept lane then knows where its bytes and its records go.
struct Prefix {
  uint32_t nvalid;      // lanes kept
  bool mine;            // this lane is one of them
  uint32_t all;         // what they produce together: bytes | records << 20
  uint32_t boff, roff;  // the bytes / records of the lanes before this one
};
template <class PF>
__device__ __forceinline__ Prefix fit_prefix(const SyncRound &r, const Sink &sk, uint32_t lane, PF &pf) {
  const uint32_t R0 = sk.pos, rb = sk.sbase();
  Prefix p;
  p.nvalid = r.nvalid;
  uint32_t mynb = lane < p.nvalid ? r.nb : 0;  // bytes | matches << 20
  const uint32_t off = wave_excl_scan(mynb, lane);
  if (p.nvalid < 64) pf.count(C_END_CHAIN);
  const uint32_t bend = ((off + mynb) & (kCountMatch - 1)), rend = (off + mynb) >> 20;
  const uint64_t fits = __ballot((R0 - rb) + bend <= STAGE - 16 && rend <= RMAX);
  const uint32_t nfit = fits == ~0ull ? 64 : (uint32_t)__builtin_ctzll(~fits);
  if (nfit < p.nvalid) {
    pf.count(rdlane(rend, nfit) > RMAX ? C_END_RECORDS : C_END_FIT);
    p.nvalid = nfit ? nfit : 1;
  }
  p.mine = lane < p.nvalid;
  if (!p.mine) mynb = 0;
  p.all = rdlane(off + mynb, p.nvalid - 1);
  p.boff = off & (kCountMatch - 1), p.roff = off >> 20;
  return p;
}

// The emit pass over the kept lanes.  Two wavefronts, one round: the copier has nothing to do until the round is emitted,
// so it emits the second half of every zone while this wavefront emits the first (the counting pass left the boundary in
// the middle and what lies before it: the halves' output positions and records are known) - the emit pass is half as
// long.  Small zones are not worth the hand-over.  False: the copier gave up.
template <bool PAIR, bool BUDGET>
__device__ __forceinline__ bool emit_round(lds_smem *sm, const Sink &sk, uint32_t lroot, uint32_t lane, uint32_t rbp, uint32_t tot,
                                           uint32_t zs, const SyncRound &r, const Prefix &p, uint32_t &sent, LaneOut &lo) {
  constexpr bool kSplit = PAIR && !BUDGET && MD_EMIT_SPLIT != 0;
  const lds_u32 *win = (const lds_u32 *)sm->win;
  const lds_u32 *lut = (const lds_u32 *)sm->lut;
  lds_u32 *mrec = (lds_u32 *)sm->mrec;
  lds_u16 *mpos = (lds_u16 *)sm->mpos;
  const uint32_t R0 = sk.pos, rb = sk.sbase();
  const uint32_t q0 = R0 + p.boff;
  lo.endp = r.end;
  lo.stopc = 0;
  lo.bytes = 0;
  lo.nm = 0;
  bool split = false;
  if constexpr (kSplit) split = zs >= 128;
  const uint32_t all = p.all & (kCountMatch - 1);  // bytes the round will produce
  const bool plain = tot >= rbp + kWave * zs + 64 && R0 >= 32768u && all <= sk.cap - R0 && (R0 - rb) + all <= STAGE - 16;
  uint32_t alimit = r.limit;
  bool gob = false;         // this lane's zone has a second half for the copier
  uint32_t bq = 0, br = 0;  // the bytes | records before it, relative to the lane's
  if constexpr (kSplit) {
    if (split) {
      gob = p.mine && r.midp != 0xffffffffu && r.midp < r.limit && r.midp >= r.start;
      bq = r.midcnt & (kCountMatch - 1);
      br = r.midcnt >> 20;
      emit_ask(sm, lane, EmitHalf{gob ? r.midp : 0xffffffffu, r.limit, q0 + bq, p.roff + br},
               EmitUni{lroot, tot, rb, R0, sk.cap, plain ? 0u : 1u});
      mail_post(sm, lane, kJobEmit, 0, 0, sent);
      alimit = gob ? r.midp : r.limit;
    }
  }
  if (plain && !BUDGET) emit_pass<false, false>(win, lut, lroot, mrec, mpos, sk.stage, p.roff, tot, p.mine, r.start, alimit, q0, rb, R0, sk.cap, lo);
  else emit_pass<true, BUDGET>(win, lut, lroot, mrec, mpos, sk.stage, p.roff, tot, p.mine, r.start, alimit, q0, rb, R0, sk.cap, lo);
  if constexpr (kSplit) {
    if (split) {
      if (!mail_wait_idle(sm, sent)) return false;
      if (gob) lo = merge_halves(lo, emit_replied(sm, lane), bq, br);
    }
  }
  return true;
}
// the copier's half of it
__device__ __forceinline__ void emit_second_halves(lds_smem *sm, const Sink &sk, uint32_t lane) {
  EmitHalf h;
  EmitUni u;
  emit_asked(sm, lane, h, u);
  const bool go = h.start != 0xffffffffu;
  LaneOut lo;
  lo.endp = h.start, lo.stopc = 0, lo.bytes = 0, lo.nm = 0;
  const lds_u32 *win = (const lds_u32 *)sm->win;
  const lds_u32 *lut = (const lds_u32 *)sm->lut;
  if (u.checked) emit_pass<true, false>(win, lut, u.lroot, (lds_u32 *)sm->mrec, (lds_u16 *)sm->mpos, sk.stage, h.rec0, u.tot, go, go ? h.start : 0u, h.limit, h.q0, u.rb, u.R0, u.cap, lo);
  else emit_pass<false, false>(win, lut, u.lroot, (lds_u32 *)sm->mrec, (lds_u16 *)sm->mpos, sk.stage, h.rec0, u.tot, go, go ? h.start : 0u, h.limit, h.q0, u.rb, u.R0, u.cap, lo);
  emit_reply(sm, lane, lo);
}

// next round: 64 zones that fill about 7/8 of the staging buffer at this round's bytes-per-bit
__device__ __forceinline__ uint32_t next_zone(uint32_t bits, uint32_t total) {
  const uint64_t want = (uint64_t)(STAGE - STAGE / 8) * bits / ((uint64_t)kWave * (total ? total : 1u));
  return want > S ? S : want < SMIN ? SMIN : (uint32_t)want;
}

// ---------------------------------------------------------------------------
// All rounds of one Huffman block.  bp is a bit position of the body; on return *bp_io is the bit after the EOB.
// PAIR: this wavefront only decodes — a round's records and literals go to the copier wavefront (copier_main), which
// copies the matches, folds the checksum and writes the round out while this one is already walking the next round's
// zones; sk is then the decoder's own idea of the output position, and `sent` counts the jobs posted.
// BUDGET: the block has an incomplete code (see sync_pass); that form is not made for speed.
template <class PF, bool PAIR, bool BUDGET>
__device__ __forceinline__ int inflate_block(lds_smem *sm, const uint8_t *__restrict__ body, uint32_t body_len, Sink &sk,
                                             uint32_t lroot, uint32_t lane, uint32_t *bp_io, uint32_t *zone_io, Window &wnd,
                                             KnownBounds &kb, uint32_t &sent, PF &pf) {
  uint32_t bp = *bp_io;
  lds_u32 *win = (lds_u32 *)sm->win;
  const lds_u32 *lut = (const lds_u32 *)sm->lut;
  const uint32_t total_bits = body_len * 8;
  uint32_t zs = *zone_io;  // zone size of this round (wave-uniform), adapted to the expansion of the last one
  constexpr bool kSplit = PAIR && !BUDGET && MD_EMIT_SPLIT != 0;
  for (;;) {
    const uint32_t base = (bp >> 5) << 2;  // window start (byte of the body, multiple of 4)
    wnd.ensure(win, body, body_len, base, lane);
    const uint32_t rbp = bp - base * 8, tot = total_bits - base * 8;  // window-relative
    pf.tick(P_ENSURE);
    pf.count(C_ROUNDS);
    SyncRound r;
    if (!kb.replay(r, rbp, zs, lane)) {
      r = sync_round<BUDGET, kSplit>(win, lut, lroot, lane, rbp, zs, pf);
      kb.record(r);
    }
    pf.tick(P_DECODE2);
    const Prefix p = fit_prefix(r, sk, lane, pf);
    if constexpr (PAIR) {  // the staging buffer and the record arrays are the copier's until it has written the last round out
      pf.tick(P_DECODE2);
      if (!mail_wait_idle(sm, sent)) return MD_E_HIP;
      pf.tick(P_WAIT_DEC);
    }
    LaneOut lo;
    if (!emit_round<PAIR, BUDGET>(sm, sk, lroot, lane, rbp, tot, zs, r, p, sent, lo)) return MD_E_HIP;
    pf.tick(P_EMIT_A);
    const Verdict v = round_verdict(p.mine, lo, p.boff, p.roff, p.nvalid, p.all & (kCountMatch - 1), p.all >> 20);
    if (v.lstop == kStEob) pf.count(C_END_EOB);
    else if (v.lstop == kStTrunc) pf.count(C_END_STAGE);
    const uint32_t nbp = base * 8 + rdlane(lo.endp, v.nvalid - 1);
    wnd.fetch(body, body_len, (nbp >> 5) << 2, lane);  // the next round's (or the next block header's) window: on its way
    bool stuck = false;
    if constexpr (PAIR) {
      mail_post(sm, lane, kJobRound, v.total, v.nrec, sent);
      sk.pos += v.total;
    } else {
      copy_round(sm, sk, lane, v.total, v.nrec, &stuck, pf);
    }
    pf.count(C_LANES, v.nvalid);
    if (stuck || (nbp == bp && v.total == 0 && (v.lstop == 0 || v.lstop == kStTrunc))) return MD_E_HIP;  // defensive: no progress
    zs = next_zone(nbp - bp, v.total);
    bp = nbp;
    if (v.lstop == kStEob) break;
    if (v.lstop != 0 && v.lstop != kStTrunc) return (int)v.lstop;
  }
  *bp_io = bp;
  *zone_io = zs;
  return MD_OK;
}

// stored bytes body[p, p + len) -> staging buffer -> output (lib/de.ml:1613-1627), a staging buffer at a time
__device__ __forceinline__ void copy_stored(Sink &sk, const uint8_t *__restrict__ body, uint32_t p, uint32_t len, uint32_t lane) {
  const uint8_t *q = body + p;
  uint32_t left = len;
  while (left) {
    const uint32_t seg = left < STAGE - 16 ? left : STAGE - 16;
    const uint32_t s0 = sk.pos - sk.sbase();
    for (uint32_t j = lane; j < seg; j += kWave) sk.stage[s0 + j] = q[j];
    sk.flush(seg);
    q += seg;
    left -= seg;
  }
}

// The copier wavefront of a stream: takes the decoder's jobs one by one until it is told to quit.
template <class PF>
__device__ __forceinline__ void copier_main(lds_smem *sm, const uint8_t *__restrict__ body, Sink &sk, uint32_t lane, PF &pf) {
  uint32_t done = 0;
  for (;;) {
    while (uni(mail_ld(&sm->mail.emitted)) == done) __builtin_amdgcn_s_sleep(2);
    asm volatile("" ::: "memory");
    const uint32_t kind = uni(sm->mail.kind), total = uni(sm->mail.total), x = uni(sm->mail.x);
    pf.tick(P_WAIT_COPY);
    if (kind == kJobQuit) break;
    bool stuck = false;
    if (kind == kJobRound) copy_round(sm, sk, lane, total, x, &stuck, pf);
    else if (kind == kJobEmit) {
      if constexpr (MD_EMIT_SPLIT != 0) emit_second_halves(sm, sk, lane);
    } else copy_stored(sk, body, x, total, lane);
    if (lane == 0) {
      sm->mail.a = sk.a;
      sm->mail.b = sk.b;
      if (stuck) sm->mail.stuck = 1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    done++;
    if (lane == 0) mail_st(&sm->mail.copied, done);
  }
}

// The decoder's side of block_loop (inflate_wave_core.hpp): a stored block's bytes are copied (PAIR: by the copier), a
// Huffman block is decoded, and a stream in pieces notes every complete block.
template <class PF, bool PAIR>
struct DecodeBlocks {
  lds_smem *sm;
  const uint8_t *body;
  uint32_t body_len, lane, sid;
  Sink &sk;
  Window &wnd;
  KnownBounds &kb;
  PF &pf;
  const Cont &cont;
  uint32_t zone;  // the next round's zone size
  uint32_t sent;  // PAIR: jobs posted
  __device__ __forceinline__ int stored(uint32_t p, uint32_t len) {
    if (len > sk.cap - sk.pos) return MD_UNEXPECTED_END_OF_OUTPUT;
    int rc = MD_OK;
    if (len) {  // (an empty stored block - a flush point - is its header and nothing else)
      if constexpr (PAIR) {
        if (!mail_wait_idle(sm, sent)) rc = MD_E_HIP;
        mail_post(sm, lane, kJobStored, len, p, sent);
        sk.pos += len;
      } else {
        copy_stored(sk, body, p, len, lane);
      }
    }
    return rc;
  }
  // (lane & 63 is lane.  The two builders are compiled on their own, and what they know of their arguments they learn at
  // the call, before this struct has dissolved into the kernel: told that lane < 64, dynamic_tables keeps one
  // callee-saved register fewer - 4 bytes of the kernel's 40 of scratch, which tests/test_inflate_resources.py caps)
  __device__ __forceinline__ void fixed(uint32_t &lroot) { fixed_tables(sm, lane & (kWave - 1), &lroot); }
  __device__ __forceinline__ int dynamic(uint32_t rbp, uint32_t tot, uint32_t &hend, uint32_t &lroot) {
    return dynamic_tables(sm, rbp, tot, lane & (kWave - 1), &hend, &lroot, pf);
  }
  __device__ __forceinline__ void header_done() { pf.tick(P_HEADER); }
  template <bool BUDGET>
  __device__ __forceinline__ int huffman(uint32_t lroot, uint32_t &bp) {
    return inflate_block<PF, PAIR, BUDGET>(sm, body, body_len, sk, lroot, lane, &bp, &zone, wnd, kb, sent, pf);
  }
  __device__ __forceinline__ void block_done(int &rc, uint32_t bp, bool last) {
    if (cont.resume_bits && rc == MD_OK) {  // the next piece of the stream could start here
      if constexpr (PAIR) {                 // (the checksum state is the copier's)
        if (!mail_wait_idle(sm, sent)) rc = MD_E_HIP;
        sk.a = uni(sm->mail.a);
        sk.b = uni(sm->mail.b);
      }
      if (lane == 0) {
        cont.resume_bits[sid] = bp;
        cont.resume_out[sid] = sk.pos;
        cont.resume_adler[sid] = (sk.b << 16) | sk.a;
        cont.resume_last[sid] = last ? 1u : 0u;
      }
    }
  }
};

// PAIR = two wavefronts per stream (decoder + copier, see inflate_block); otherwise one wavefront does both in turn.
// a.cont: a stream decoded in pieces (struct Cont, internal.hpp), all null for whole streams.
template <bool PROF, bool PAIR>
__global__ __launch_bounds__(PAIR ? 2 * kWave : kWave, PAIR ? MD_PAIR_OCC : 2) void inflate_wave_kernel(const InfArgs a) {
  __shared__ Smem smem;  // static: LDS addresses fold into the instructions' offset fields
  lds_smem *sm = (lds_smem *)&smem;
  Prof<PROF> pf;
  pf.init();
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t wave = PAIR ? uni(threadIdx.x / kWave) : 0u;  // 0 = decoder, 1 = copier
  if (blockIdx.x >= a.n) return;
  const uint32_t sid = a.order ? a.order[blockIdx.x] : blockIdx.x;  // workgroups start in index order: longest streams first
  const int format = a.format;
  uint64_t *const out_len = a.out_len, *const consumed = a.consumed, *const dbg = a.dbg;
  int32_t *const status = a.status;
  uint32_t *const checksum = a.checksum;
  const Cont &cont = a.cont;

  const uint8_t *src = a.in + a.in_off[sid];
  const uint64_t cap64 = a.out_cap[sid];
  const Opened o = open_stream(format, src, a.in_len[sid]);
  if (o.rc == MD_E_INVALID_ARGUMENT) {
    if (threadIdx.x == 0) {
      out_len[sid] = 0;
      consumed[sid] = 0;
      status[sid] = MD_E_INVALID_ARGUMENT;
      if (checksum) checksum[sid] = 0;
    }
    return;
  }
  const bool cap_clamped = cap64 > MD_MAX_STREAM;  // more room than 32-bit cursors can use
  const uint32_t cap = cap_clamped ? (uint32_t)MD_MAX_STREAM : (uint32_t)cap64;
  int rc = o.rc;
  const uint32_t body_len = o.body_len;
  const uint8_t *body = src + o.body_off;

  Sink sk;  // PAIR: the copier's is the real one, the decoder's only follows the output position
  sk.stage = (lds_u8 *)sm->stage;
  sk.g = a.out + a.out_off[sid];
  sk.cap = cap;
  const uint32_t hist = cont.hist_len ? cont.hist_len[sid] : 0u, adler0 = cont.adler_in ? cont.adler_in[sid] : 1u;
  sk.pos = hist < cap ? hist : cap;  // (the history is the caller's: it fits the buffer)
  sk.lane = lane;
  sk.a = adler0 & 0xffffu;
  sk.b = adler0 >> 16;
  sk.want_adler = (checksum != nullptr) || format == MD_FORMAT_ZLIB || cont.resume_adler != nullptr;

  if (threadIdx.x < 4) sm->lut[kStopEobI + threadIdx.x] = mk_entry(0, 0, 0, 0, kStopEobI + (threadIdx.x & 2));  // the self-looping STOP entries
  if constexpr (PAIR) {
    if (threadIdx.x < sizeof(Mail) / 4) ((lds_u32 *)&sm->mail)[threadIdx.x] = threadIdx.x == 6 ? sk.a : threadIdx.x == 7 ? sk.b : 0u;
    __syncthreads();
    if (wave == 1) {
      copier_main(sm, body, sk, lane, pf);
      if constexpr (PROF) {
        if (lane == 0 && sid == 0 && dbg) {
          const int mine[] = {P_FAR, P_NEAR, P_ADLER, P_NEAR_FAST, P_NEAR_SLOW, P_NEAR_UPD, P_NEAR_LOAD, P_FAR_REC, P_FAR_LOAD, P_WAIT_COPY};
          for (int i : mine) dbg[i] = pf.acc[i];
          dbg[P_COUNT + C_NEAR_IT] = pf.cnt[C_NEAR_IT];
          dbg[P_COUNT + C_LONG_NEAR] = pf.cnt[C_LONG_NEAR];
          dbg[P_COUNT + C_FAR_SPILL] = pf.cnt[C_FAR_SPILL];
        }
      }
      return;
    }
  }

  uint32_t bp = cont.start_bit ? cont.start_bit[sid] & 7u : 0u;
  Window wnd;
  wnd.base = 0xffffffffu;
  KnownBounds kb;
  kb.init(sid);
  if (cont.resume_bits && lane == 0) {  // no block complete yet
    cont.resume_bits[sid] = bp;
    cont.resume_out[sid] = sk.pos;
    cont.resume_adler[sid] = adler0;
    cont.resume_last[sid] = 0;
  }

  DecodeBlocks<Prof<PROF>, PAIR> h = {sm, body, body_len, lane, sid, sk, wnd, kb, pf, cont, S, 0};
  if (rc == MD_OK) rc = block_loop(h, sm, body, body_len, lane, bp, wnd);
  if constexpr (PAIR) {  // everything posted is written out; the checksum state comes back, the copier goes home
    if (!mail_wait_idle(sm, h.sent) && rc == MD_OK) rc = MD_E_HIP;
    sk.a = uni(sm->mail.a);
    sk.b = uni(sm->mail.b);
    mail_post(sm, lane, kJobQuit, 0, 0, h.sent);
  }
  uint32_t used = (bp + 7) >> 3;  // i_pos - (bits lsr 3), lib/de.ml:1805
  uint32_t adler = (sk.b << 16) | sk.a;
  if (rc == MD_OK && format == MD_FORMAT_ZLIB) {
    const uint8_t *t = src + 2 + used;
    uint32_t want = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
    if (want != adler) rc = MD_INVALID_CHECKSUM;
    used += 6;
  }
  if (rc == MD_UNEXPECTED_END_OF_OUTPUT && cap_clamped) rc = MD_E_INVALID_ARGUMENT;  // a > 4 GiB stream
  if (lane == 0) {
    out_len[sid] = sk.pos;
    consumed[sid] = rc == MD_OK ? used : 0;
    status[sid] = rc;
    if (checksum) checksum[sid] = adler;
  }
  if constexpr (PROF) {
    if (lane == 0 && sid == 0 && dbg) {
      if constexpr (PAIR) {
        const int mine[] = {P_ENSURE, P_DECODE1, P_DECODE2, P_EMIT_A, P_HEADER, P_HDR_LENS, P_HDR_LIT, P_WAIT_DEC};
        for (int i : mine) dbg[i] = pf.acc[i];
        for (int i = 0; i < C_COUNT; i++)
          if (i != C_NEAR_IT && i != C_LONG_NEAR && i != C_FAR_SPILL) dbg[P_COUNT + i] = pf.cnt[i];
      } else {
        for (int i = 0; i < P_COUNT; i++) dbg[i] = pf.acc[i];
        for (int i = 0; i < C_COUNT; i++) dbg[P_COUNT + i] = pf.cnt[i];
      }
    }
  }
}

// Launch order of a batch: a stream's time grows with its compressed length, and a batch of more streams than the
// chip holds at once (8 per CU) ends when its last wavefront does.  Workgroups are started in index order, so the
// streams are handed out longest first (256 length classes, counting sort; the order inside a class is whatever
// the atomics give — nothing a stream computes depends on it).
constexpr uint32_t kOrderThreads = 1024, kOrderClasses = 256;
__global__ __launch_bounds__(kOrderThreads) void inflate_order_kernel(uint32_t n, const uint64_t *__restrict__ in_len,
                                                                      uint32_t *__restrict__ order) {
  __shared__ uint32_t cls[kOrderClasses];
  __shared__ uint32_t longest;
  const uint32_t t = threadIdx.x;
  if (t < kOrderClasses) cls[t] = 0;
  if (t == 0) longest = 0;
  __syncthreads();
  uint32_t m = 0;
  for (uint32_t i = t; i < n; i += kOrderThreads) {
    const uint64_t l = in_len[i];
    const uint32_t l32 = l > MD_MAX_INFLATE_IN ? 0u : (uint32_t)l;  // rejected at once by the kernel
    m = l32 > m ? l32 : m;
  }
  atomicMax(&longest, m);
  __syncthreads();
  const uint64_t span = (uint64_t)longest + 1;
  auto klass = [&](uint32_t i) {
    const uint64_t l = in_len[i];
    const uint32_t l32 = l > MD_MAX_INFLATE_IN ? 0u : (uint32_t)l;
    return (kOrderClasses - 1) - (uint32_t)((uint64_t)l32 * kOrderClasses / span);  // class 0 = the longest
  };
  for (uint32_t i = t; i < n; i += kOrderThreads) atomicAdd(&cls[klass(i)], 1u);
  __syncthreads();
  if (t == 0) {  // exclusive scan of 256 counters
    uint32_t acc = 0;
    for (uint32_t c = 0; c < kOrderClasses; c++) {
      const uint32_t v = cls[c];
      cls[c] = acc;
      acc += v;
    }
  }
  __syncthreads();
  for (uint32_t i = t; i < n; i += kOrderThreads) order[atomicAdd(&cls[klass(i)], 1u)] = i;
}

}  // namespace wv
}  // namespace md

// the launch order of a batch (longest first) on its own: the deflate kernels take it too
extern "C" int md_launch_stream_order(uint32_t n, const uint64_t *in_len, uint32_t *order, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(md::wv::inflate_order_kernel, dim3(1), dim3(md::wv::kOrderThreads), 0, stream, n, in_len, order);
  return (int)hipGetLastError();
}

// measurement only (md_set_option "debug_inflate_lds_pad", tools/dbg/inflate_occupancy.py): bytes of unused dynamic LDS
// per workgroup, which lowers the number of streams a CU holds at once
static uint32_t g_debug_lds_pad = 0;
extern "C" int md_i_debug_inflate_lds_pad(uint32_t bytes) {
  using namespace md::wv;
  if (bytes + sizeof(Smem) > 160u * 1024u) return 1;
  hipError_t e = hipFuncSetAttribute((const void *)inflate_wave_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)inflate_wave_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return (int)e;
  g_debug_lds_pad = bytes;
  return 0;
}

extern "C" int md_i_debug_known_bounds(int mode, uint32_t nstreams) {
#ifdef MD_DEBUG_KNOWN_BOUNDS
  static uint4 *buf = nullptr;
  static uint32_t cap = 0;
  if (nstreams > cap) {
    if (buf) hipFree(buf);
    if (hipMalloc((void **)&buf, (size_t)nstreams * md::wv::KB_ROUNDS * 64 * sizeof(uint4)) != hipSuccess) return 2;
    cap = nstreams;
    if (hipMemcpyToSymbol(HIP_SYMBOL(md::wv::g_kb_buf), &buf, sizeof buf) != hipSuccess) return 3;
  }
  return hipMemcpyToSymbol(HIP_SYMBOL(md::wv::g_kb_mode), &mode, sizeof mode) == hipSuccess ? 0 : 4;
#else
  (void)mode, (void)nstreams;
  return 1;  // not a measurement build
#endif
}

template <bool PROF, bool PAIR>
static void launch_inflate(const md::wv::InfArgs &a, hipStream_t stream) {
  using namespace md::wv;
  hipLaunchKernelGGL((inflate_wave_kernel<PROF, PAIR>), dim3(a.n), dim3(PAIR ? 2 * kWave : kWave), PROF ? 0u : g_debug_lds_pad, stream, a);
}
extern "C" int md_launch_inflate_wave(const md::wv::InfArgs *args, hipStream_t stream) {
  if (args->n == 0) return 0;
  using namespace md::wv;
  InfArgs a = *args;
  if (a.order) hipLaunchKernelGGL(inflate_order_kernel, dim3(1), dim3(kOrderThreads), 0, stream, a.n, a.in_len, a.order);
  if (a.dbg) a.order = nullptr;      // (a profiled launch runs in index order)
  const bool single = a.waves == 1;  // the one-wavefront form of the kernel: same results, kept for comparison
  if (a.dbg) single ? launch_inflate<true, false>(a, stream) : launch_inflate<true, true>(a, stream);
  else single ? launch_inflate<false, false>(a, stream) : launch_inflate<false, true>(a, stream);
  return (int)hipGetLastError();
}
