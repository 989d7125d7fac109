// inflate_wave_core.hpp — what the batch inflate kernel (inflate_wave.hip) and the size-query kernel (inflate_count.hip)
// share: the geometry of a round, the walk table and its builders, the input window, the block-header parser and the
// walks.  Device code, included by exactly those two files; each compiles its own copy, so neither kernel's code depends
// on the other's callers.  The description of the decoder is at the head of inflate_wave.hip.
#pragma once
#include <stdlib.h>
#include "inflate_util.hpp"
#include "internal.hpp"

#if !defined(MD_RMAX) || !defined(MD_STAGE)
#error "define MD_RMAX and MD_STAGE before inflate_wave_core.hpp"
#endif

namespace md {
namespace wv {

// ---- geometry ---------------------------------------------------------------------------------
constexpr uint32_t S = 264;        // bits per lane zone at most: 8.25 dwords, so the 64 cursors start on distinct LDS banks
constexpr uint32_t SMIN = 48;      // ... and at least: where the data expands so much that 64 full zones overflow the
                                   // staging buffer, the zones shrink so that all 64 lanes still have work (cost then
                                   // follows the output, not the number of zones thrown away)
constexpr uint32_t KMAX = 64;      // walk steps per lane per pass
#ifndef MD_EMIT_SPLIT
#define MD_EMIT_SPLIT 1  // the two wavefronts of a stream emit a round together, each one half of every zone (inflate_block)
#endif
#if defined(MD_DEBUG_KNOWN_BOUNDS)
#undef MD_EMIT_SPLIT
#define MD_EMIT_SPLIT 0  // (the replayed sync results carry no mid-zone boundaries)
#endif
#ifndef MD_SPLIT_B
#define MD_SPLIT_B 4  // eighths of a zone that the copier emits
#endif
#ifndef MD_RUNIN_NUM
#define MD_RUNIN_NUM 3
#define MD_RUNIN_DEN 2
#endif
constexpr uint32_t RUNIN_NUM = MD_RUNIN_NUM, RUNIN_DEN = MD_RUNIN_DEN;  // run-in of the speculative pass, as a fraction of the zone
constexpr uint32_t PASSES = 5;     // walks after the first one: at least this many are allowed, more when the zones are small
constexpr uint32_t PASS_BITS = 1600, PASSES_MAX = 16;  // (a walk costs in proportion to the zone size)
// (MD_RMAX, MD_STAGE: the including file's; they size the tail of Smem, behind the window and the table)
constexpr uint32_t RMAX = MD_RMAX;     // match records per round, all lanes together (in stream order)
constexpr uint32_t STAGE = MD_STAGE;   // staging bytes (one round of output)
constexpr uint32_t WIN_WORDS = 544;  // input window: 31 + 64*S + 47 bits and the two words a peek touches

// LUT entry: n[4:0] | xb[8:5] | val8[16:9] | next.nbits[20:17] | next.tb[31:21]
//   n      bits this step consumes: the code (a LINK entry: the root bits, the sub-table entry behind it: the rest of
//          the code) and the extra bits that follow it
//   xb     how many of them are extra bits (the last xb of the n)
//   val8   literal byte | length base - 3 (0..255) | distance base m (0..3), base = (m << xb) + 1
//   next   the table the following step indexes: the lit/len root, the distance root, a sub-table (this is a LINK
//          entry then), or one of the two self-looping STOP entries (end of block / no such code)
// The tables lie in this order: lit/len sub-tables, distance root and sub-tables, lit/len root, the STOP entries -
// and every table starts on an EVEN entry.  So (1) `e >> 17` has the next index width in its low FIVE bits (what
// v_bfe_u32 takes as its width operand) and `e >> 21` is the next table: a step needs no masks; (2) "this step ended a
// token at or beyond `lim`, or ran into a STOP entry" is ONE unsigned compare: (e & kTbMask) | p >= (kLitB << 21) | lim.
constexpr uint32_t kLitSize = 852, kDistSize = 592;  // zlib ENOUGH (lib/de.ml:579-580)
constexpr uint32_t kLitRootMax = 512;                // the lit/len root is at most 9 bits wide (De.Inf.huffman's root)
constexpr uint32_t kLitSubB = 0;                     // lit/len sub-tables: they exist only behind a 9-bit root
constexpr uint32_t kDistB = kLitSize - kLitRootMax;  // 340
constexpr uint32_t kLitB = kDistB + kDistSize;       // 932
constexpr uint32_t kStopEobI = kLitB + kLitRootMax;  // 1444
constexpr uint32_t kStopBadI = kStopEobI + 2;
constexpr uint32_t kLutWords = kStopBadI + 2;
constexpr uint32_t kTbMask = 0xffe00000u;
constexpr uint32_t kLoopy = 0x100u;  // with the root width of a block: an incomplete code, a walk can stand still
static_assert(kDistB % 2 == 0 && kLitB % 2 == 0 && kStopEobI % 2 == 0 && kLutWords == 1448, "even table bases");
constexpr uint32_t kStEob = 100, kStTrunc = 101;  // lane stop reasons; < 100 = MD_* status
constexpr uint32_t kCountMatch = 1u << 20;         // a walk counts bytes | matches << 20 (64 lanes: < 2^20 bytes, < 2^12 matches)
constexpr uint32_t kNearBit = 0x8000u;            // match record: len-3[23:16] | near[15] | dist-1[14:0]
__device__ __forceinline__ uint32_t rec_dist(uint32_t tk) { return (tk & 0x7fff) + 1; }
__device__ __forceinline__ uint32_t rec_len(uint32_t tk) { return ((tk >> 16) & 0xff) + 3; }

// The two wavefronts of a stream talk through this: the decoder posts jobs, the copier reports them done.  A wavefront's
// LDS operations execute in order, so a job's records and literals are in LDS before `emitted` says so, and the
// copier's last read of them is over before `copied` does.
struct Mail {
  uint32_t emitted;  // jobs posted by the decoder
  uint32_t copied;   // jobs finished by the copier: staging buffer and records are free again
  uint32_t kind;     // kJobRound | kJobStored | kJobQuit | kJobEmit
  uint32_t total;    // bytes the job produces
  uint32_t x;        // match records of the round | body offset of the stored bytes
  uint32_t stuck;    // the copier's defensive verdict
  uint32_t a, b;     // Adler-32 state after job `copied`
};
constexpr uint32_t kJobRound = 0, kJobStored = 1, kJobQuit = 2, kJobEmit = 3;
// kJobEmit: the copier emits the second halves of the round's zones while the decoder emits the first ones.  What it needs
// lies in `list` (the copier's own array, idle between two rounds): four words per lane, then six wave-uniform words; the
// lanes' results come back in the same place (struct EmitJob, inflate_wave.hip).
constexpr uint32_t kHxUni = 4 * 64;  // word index of the uniform part
struct Smem {  // the kernel's only LDS object: it sits at LDS address 0
  uint32_t win[WIN_WORDS];
  uint32_t lut[kLutWords];
  uint32_t mrec[RMAX];                     // the round's match records in stream order
  uint16_t mpos[RMAX];                     // their staging positions
  alignas(16) uint8_t stage[STAGE + 16];   // one round of output; header scratch while a header is parsed
  uint16_t list[RMAX];                     // the round's near matches (indices into mrec), in stream order
  Mail mail;
};
struct HScratch {       // aliases the tail of Smem::win (hscratch_of)
  uint8_t lens[384];    // code lengths: lit/len symbols, then the distance symbols
  uint16_t work[320];   // symbols sorted by (code length, symbol)
  uint32_t ctr;         // sub-table allocation counter
};
#if MD_RMAX == 576 && MD_STAGE == 5248
static_assert(sizeof(Smem) <= 17920, "9 streams (18 wavefronts) per CU: 160 KiB / 9, in whole 512-byte units");
#endif
static_assert(RMAX % 64 == 0 && STAGE % 16 == 0 && RMAX * 2 >= (kHxUni + 6) * 4, "record rows, staging chunks, the emit job's words in `list`");
// A dynamic header is at most 17 + 19 x 3 + 320 x 14 bits = 570 bytes and starts in the window's first word: the window's
// tail is free while a header is parsed (the staging buffer is not: the copier wavefront may still be writing a round out)
constexpr uint32_t kHScratchAt = 1136;
static_assert(kHScratchAt >= 4 + 572 + 8 && kHScratchAt % 16 == 0 && kHScratchAt + sizeof(HScratch) <= WIN_WORDS * 4, "header scratch lives behind the header's bits");
typedef MD_LDS Smem lds_smem;
typedef MD_LDS HScratch lds_hscratch;
__device__ __forceinline__ lds_hscratch *hscratch_of(lds_smem *sm) {
  return reinterpret_cast<lds_hscratch *>(reinterpret_cast<lds_u8 *>(sm->win) + kHScratchAt);
}

__device__ __forceinline__ uint32_t mk_entry(uint32_t n, uint32_t xb, uint32_t val8, uint32_t nbits, uint32_t tb) {
  return n | (xb << 5) | (val8 << 9) | (nbits << 17) | (tb << 21);
}
__device__ __forceinline__ uint32_t e_n(uint32_t e) { return e & 31; }
__device__ __forceinline__ uint32_t e_xb(uint32_t e) { return (e >> 5) & 15; }
__device__ __forceinline__ uint32_t e_val(uint32_t e) { return (e >> 9) & 255; }
__device__ __forceinline__ uint32_t e_tb(uint32_t e) { return e >> 21; }
// a LINK entry leads to a sub-table: neither a root nor a STOP entry
__device__ __forceinline__ bool e_link(uint32_t e) { return e_tb(e) < kLitB && e_tb(e) != kDistB; }
// the state a walk starts in: "the next step indexes the lit/len root"
__device__ __forceinline__ uint32_t e_root(uint32_t lroot) { return mk_entry(0, 0, 0, lroot, kLitB); }
// leaf entries; `codelen` = bits of the code this step consumes
__device__ __forceinline__ uint32_t lit_leaf(uint32_t sym, uint32_t codelen, uint32_t lroot, uint32_t droot) {
  if (sym < 256) return mk_entry(codelen, 0, sym, lroot, kLitB);
  if (sym == 256) return mk_entry(codelen, 0, 0, 0, kStopEobI);
  const uint32_t l = (sym - 257) & 31;  // lib/de.ml:293-311 (29,30 -> length 3)
  const uint32_t xb = (l >= 8 && l < 28) ? (l - 4) >> 2 : 0;
  const uint32_t base3 = l < 8 ? l : l < 28 ? (4 + (l & 3)) << xb : l == 28 ? 255 : 0;  // length base - 3
  return mk_entry(codelen + xb, xb, base3, droot, kDistB);
}
// a distance leaf carries the base of its symbol as `m`, base = (m << xb) + 1: m = the symbol itself for 0..3, 2 or 3
// for 4..29 (lib/de.ml:313-325); the invalid symbols 30 and 31 lead to the STOP entry of "no such code" and, unlike an
// empty table slot, consume their code (slow_token tells them apart by that)
__device__ __forceinline__ uint32_t dist_leaf(uint32_t dv, uint32_t codelen, uint32_t lroot) {
  dv &= 31;
  if (dv >= 30) return mk_entry(codelen, 0, 0, 0, kStopBadI);
  const uint32_t xb = dv >= 4 ? (dv - 2) >> 1 : 0;
  const uint32_t m = dv < 4 ? dv : ((dv & 1) | 2);
  return mk_entry(codelen + xb, xb, m, lroot, kLitB);
}
// leaf value + extra bits -> distance (lib/de.ml:321-325, +1 folded in)
__device__ __forceinline__ uint32_t dist_value(uint32_t m, uint32_t xb, uint32_t x) { return (m << xb) + 1 + x; }

// ---- input window -----------------------------------------------------------------------------
// The window holds body bytes [base, base + 4*WIN_WORDS), base a multiple of 4; zero beyond the body.  A lane loads
// 32 bytes of it (and the first lanes one more word): fetch() starts the loads into registers, put() stores them to
// LDS.  A round fetches the window of the next one as soon as it knows where that begins: the loads are in flight
// while the round is handed over (or copied).
struct Window {
  uint32_t w[8], wx;
  uint32_t base;  // of the fetched words; 0xffffffff = nothing fetched
  __device__ __forceinline__ void fetch(const uint8_t *__restrict__ body, uint32_t nbytes, uint32_t b, uint32_t lane) {
    base = b;
    const uint32_t off = b + lane * 32;
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = 0;
    if (off + 32 <= nbytes) __builtin_memcpy(w, body + off, 32);
    else if (off < nbytes)
      for (uint32_t k = 0; k < 32 && off + k < nbytes; k++) w[k >> 2] |= (uint32_t)body[off + k] << (8 * (k & 3));
    wx = 0;
    if (lane < WIN_WORDS - 512) {
      const uint32_t ox = b + 2048 + lane * 4;
      if (ox + 4 <= nbytes) __builtin_memcpy(&wx, body + ox, 4);
      else if (ox < nbytes)
        for (uint32_t k = 0; k < 4 && ox + k < nbytes; k++) wx |= (uint32_t)body[ox + k] << (8 * k);
    }
  }
  __device__ __forceinline__ void put(lds_u32 *win, uint32_t lane) const {
    lds_u32 *dst = win + lane * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = w[k];
    if (lane < WIN_WORDS - 512) win[512 + lane] = wx;
  }
  // the window at `b` in LDS, from the fetched words if they are the right ones
  __device__ __forceinline__ void ensure(lds_u32 *win, const uint8_t *__restrict__ body, uint32_t nbytes, uint32_t b, uint32_t lane) {
    if (base != b) fetch(body, nbytes, b, lane);
    put(win, lane);
    base = 0xffffffffu;
  }
};
// 32 bits of the window starting at window-relative bit position p
__device__ __forceinline__ uint32_t peek(const lds_u32 *win, uint32_t p) {
  const lds_u32 *q = reinterpret_cast<const lds_u32 *>(reinterpret_cast<const lds_u8 *>(win) + ((p >> 3) & ~3u));
  return __builtin_amdgcn_alignbit(q[1], q[0], p & 31);
}
__device__ __forceinline__ uint32_t lut_at(const lds_u32 *lut, uint32_t tb, uint32_t idx) {
  return *reinterpret_cast<const lds_u32 *>(reinterpret_cast<const lds_u8 *>(lut) + ((tb + idx) << 2));
}

// wave-uniform bit cursor over the window (block headers); values live in SGPRs
struct UBits {
  const lds_u32 *win;
  uint64_t buf;
  uint32_t n;   // valid bits in buf
  uint32_t wp;  // next window word
  __device__ __forceinline__ void init(const lds_u32 *w, uint32_t bp) {
    win = w;
    wp = bp >> 5;
    buf = ((uint64_t)uni(win[wp]) | ((uint64_t)uni(win[wp + 1]) << 32)) >> (bp & 31);
    n = 64 - (bp & 31);
    wp += 2;
  }
  __device__ __forceinline__ uint32_t pos() const { return wp * 32 - n; }
  __device__ __forceinline__ void fill() {  // afterwards n > 32
    if (n <= 32) {
      buf |= (uint64_t)uni(win[wp]) << n;
      n += 32;
      wp++;
    }
  }
  __device__ __forceinline__ uint32_t peekb(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1); }
  __device__ __forceinline__ void drop(uint32_t k) {
    buf >>= k;
    n -= k;
  }
};

// ---- Huffman tables from the canonical code ---------------------------------------------------
// De.Inf.huffman (lib/de.ml:523-638) accepts a set of code lengths iff it is not over-subscribed and
// is complete (or is a single 1-bit code, for the lit/len and distance alphabets), and then decodes
// the canonical prefix code; zlib's table layout is an implementation detail except for its size
// (documented divergence D3: more than ENOUGH entries => Invalid_dictionary).  All lanes build the
// walk table directly: per-length counts by ballot, codes by rank, root slots by a canonical search,
// sub-tables sized by the longest code behind each root slot (what zlib's `curr` loop computes for a
// complete code).
struct Canon {
  uint32_t cnt[16];    // codes per length
  uint32_t first[16];  // first canonical code (MSB first) per length
  uint32_t offs[16];   // rank of the first symbol of that length in `work`
  uint32_t max, min, root, left;
};
__device__ __forceinline__ uint32_t lane_rank(uint64_t m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}
template <int K>
__device__ __forceinline__ void canon_counts(const uint32_t (&len)[K], uint32_t rootpref, Canon &c) {
#pragma unroll
  for (int l = 1; l < 16; l++) {
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < K; k++) n += (uint32_t)__builtin_popcountll(__ballot(len[k] == (uint32_t)l));
    c.cnt[l] = n;
  }
  c.cnt[0] = 0;
  c.max = 0;
  c.min = 16;
#pragma unroll
  for (int l = 15; l >= 1; l--) {
    if (c.cnt[l] && c.max == 0) c.max = l;
    if (c.cnt[l]) c.min = l;
  }
  int left = 1;
  bool over = false;
  uint32_t code = 0, off = 0;
  c.first[0] = 0;
  c.offs[0] = 0;
#pragma unroll
  for (int l = 1; l < 16; l++) {
    left = (left << 1) - (int)c.cnt[l];
    over = over || left < 0;
    code = (code + c.cnt[l - 1]) << 1;
    c.first[l] = code;
    c.offs[l] = off;
    off += c.cnt[l];
  }
  c.left = over ? 0xffffffffu : (uint32_t)left;  // 0xffffffff = over-subscribed
  uint32_t root = rootpref;
  if (root > c.max) root = c.max;
  if (root < c.min) root = c.min;
  c.root = root;
}

// Builds one walk table: its root into lut[tb0 ..), its sub-tables into lut[sub0 ..).  len[k] = code length of symbol
// lane + 64k (0 beyond the alphabet).  LEAF(sym, codelen) encodes a leaf.  Returns false when the table would need
// more than `size` entries (D3).
template <int K, class LEAF>
__device__ __forceinline__ bool build_walk(const uint32_t (&len)[K], const Canon &c, lds_u32 *lut, uint32_t tb0, uint32_t sub0,
                                           uint32_t size, lds_hscratch *hs, uint32_t lane, uint32_t zero_entry, LEAF leaf) {
  const uint32_t root = c.root, rmask = (1u << root) - 1;
  // codes by rank inside their length class; symbols sorted by (length, symbol) for the root search
  uint32_t rev[K];
#pragma unroll
  for (int k = 0; k < K; k++) rev[k] = 0;
#pragma unroll
  for (int l = 1; l < 16; l++) {
    if (c.cnt[l]) {
      uint32_t base = 0;
#pragma unroll
      for (int k = 0; k < K; k++) {
        const uint64_t m = __ballot(len[k] == (uint32_t)l);
        if (len[k] == (uint32_t)l) {
          const uint32_t rank = base + lane_rank(m);
          rev[k] = __brev(c.first[l] + rank) >> (32 - l);
          hs->work[c.offs[l] + rank] = (uint16_t)(lane + 64 * k);
        }
        base += (uint32_t)__builtin_popcountll(m);
      }
    }
  }
  const uint32_t nroot = 1u << root;
  for (uint32_t i = lane; i < nroot; i += kWave) lut[tb0 + i] = 0;
  if (lane == 0) hs->ctr = 0;
  // longest code behind each root slot that leads to a sub-table
  if (c.max > root) {
#pragma unroll
    for (int k = 0; k < K; k++)
      if (len[k] > root)
        __hip_atomic_fetch_max(&lut[tb0 + (rev[k] & rmask)], len[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  // root slots: a link (sub-tables get their place from an LDS counter) or the leaf found by canonical search
  for (uint32_t i = lane; i < nroot; i += kWave) {
    const uint32_t v = lut[tb0 + i];
    uint32_t e;
    if (v) {
      const uint32_t sub = v - root;
      const uint32_t off = __hip_atomic_fetch_add(&hs->ctr, 1u << sub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      e = mk_entry(root, 0, 0, sub, (sub0 + off) & 2047);  // (sub-table sizes are even, so are their places)
    } else {
      const uint32_t cw = __brev(i) >> (32 - root);  // the root bits as an MSB-first code prefix
      uint32_t fl = 0, ft = 0;
#pragma unroll
      for (int l = 15; l >= 1; l--) {  // at most one length matches in a prefix code
        if (c.cnt[l] && (uint32_t)l <= root) {
          const uint32_t t = (cw >> (root - l)) - c.first[l];
          if (t < c.cnt[l]) {
            fl = l;
            ft = c.offs[l] + t;
          }
        }
      }
      e = fl ? leaf((uint32_t)hs->work[ft], fl) : zero_entry;
    }
    lut[tb0 + i] = e;
  }
  const uint32_t used = nroot + uni(hs->ctr);
  if (used > size) return false;  // D3
  // sub-table entries
  if (c.max > root) {
#pragma unroll
    for (int k = 0; k < K; k++) {
      if (len[k] > root) {
        const uint32_t link = lut[tb0 + (rev[k] & rmask)];
        const uint32_t sub = (link >> 17) & 15, tb = link >> 21;
        const uint32_t e = leaf(lane + 64 * k, len[k] - root);
        for (uint32_t j = rev[k] >> root; j < (1u << sub); j += 1u << (len[k] - root)) lut[tb + j] = e;
      }
    }
  }
  return true;
}

// the order of the code-length code lengths (lib/de.ml:225-231), 5 bits each
constexpr uint64_t kZig0 = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                           10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
constexpr uint64_t kZig1 = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;

// Dynamic block header (lib/de.ml:1733-1793) at window bit `bp`.  On MD_OK the walk tables are in lut,
// *lroot_out is the index width of the lit/len root table and *bp_out the bit after the header.
// *lroot_out also says (bit 8) that one of the two codes is incomplete: a walk over its zero entries needs a step budget.
template <class PF>
__device__ __noinline__ int dynamic_tables(lds_smem *sm, uint32_t bp_arg, uint32_t tot_arg, uint32_t lane, uint32_t *bp_out,
                                           uint32_t *lroot_out, PF &pf) {
  // arguments of a function arrive in vector registers: say that these two are wave-uniform, or the whole header
  // parse below is compiled as divergent vector code instead of scalar code
  const uint32_t bp = uni(bp_arg), tot = uni(tot_arg);
  const lds_u32 *win = (const lds_u32 *)sm->win;
  lds_hscratch *hs = hscratch_of(sm);
  UBits ub;
  ub.init(win, bp);
  if ((int32_t)(tot - ub.pos()) < 14) return MD_UNEXPECTED_END_OF_INPUT;
  const uint32_t hlit = ub.peekb(5) + 257;
  ub.drop(5);
  const uint32_t hdist = ub.peekb(5) + 1;
  ub.drop(5);
  const uint32_t hclen = ub.peekb(4) + 4;
  ub.drop(4);
  // code-length code lengths: lane j holds the length of symbol j
  uint32_t cl[1] = {0};
  for (uint32_t i = 0; i < hclen; i++) {
    ub.fill();
    if ((int32_t)(tot - ub.pos()) < 3) return MD_UNEXPECTED_END_OF_INPUT;
    const uint32_t v = ub.peekb(3);
    ub.drop(3);
    const uint32_t z = (uint32_t)((i < 12 ? kZig0 >> (5 * i) : kZig1 >> (5 * (i - 12))) & 31);
    if (lane == z) cl[0] = v;
  }
  // its decode table: 128 direct entries (root 7 >= longest code), two per lane: sym | len << 8, 0xffff = unreachable
  Canon cc;
  canon_counts<1>(cl, 7, cc);
  uint32_t cmaxl, t_lo, t_hi;
  if (cc.max == 0) {  // empty_table (lib/de.ml:521): a 1-bit code for symbol 0, the other slot out of bounds (D2)
    cmaxl = 1;
    t_lo = lane == 0 ? (1u << 8) : 0xffffu;
    t_hi = 0xffffu;
  } else {
    if (cc.left != 0) return MD_INVALID_DICTIONARY;  // over-subscribed or incomplete
    cmaxl = cc.max;
    // rank of each symbol inside its length class, then the table by canonical search (codes <= 7 bits)
#pragma unroll
    for (int l = 1; l < 8; l++) {
      const uint64_t m = __ballot(cl[0] == (uint32_t)l);
      if (cl[0] == (uint32_t)l) hs->work[cc.offs[l] + lane_rank(m)] = (uint16_t)lane;
    }
    uint32_t t[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t i = lane + 64 * h;
      const uint32_t cw = __brev(i & ((1u << cmaxl) - 1)) >> (32 - cmaxl);
      uint32_t fl = 0, ft = 0;
#pragma unroll
      for (int l = 7; l >= 1; l--) {
        if (cc.cnt[l] && (uint32_t)l <= cmaxl) {
          const uint32_t x = (cw >> (cmaxl - l)) - cc.first[l];
          if (x < cc.cnt[l]) {
            fl = l;
            ft = cc.offs[l] + x;
          }
        }
      }
      t[h] = fl ? ((uint32_t)hs->work[ft] | (fl << 8)) : 0xffffu;
    }
    t_lo = t[0];
    t_hi = t[1];
  }
  // the hlit + hdist code lengths, run-length coded (lib/de.ml:1733-1769)
  const uint32_t max_res = hlit + hdist;
  for (uint32_t x = lane; x < 384; x += kWave) hs->lens[x] = 0;
  // One scalar step per symbol.  With enough input left for the longest header there can be (316 symbols of 7 + 7
  // bits) the end-of-input tests are left out of the loop.
  auto run_lengths = [&](auto checked) -> int {
    constexpr bool CHECK = decltype(checked)::value;
    uint32_t i = 0, prev = 0;
    while (i < max_res) {
      ub.fill();
      if (CHECK && (int32_t)(tot - ub.pos()) < (int32_t)cmaxl) return MD_UNEXPECTED_END_OF_INPUT;
      const uint32_t idx = ub.peekb(cmaxl);
      const uint32_t e_lo = __builtin_amdgcn_readlane(t_lo, idx & 63), e_hi = __builtin_amdgcn_readlane(t_hi, idx & 63);
      const uint32_t e = idx < 64 ? e_lo : e_hi;
      if (e == 0xffffu) return MD_INVALID_DICTIONARY;
      const uint32_t sym = e & 0xff;
      ub.drop(e >> 8);
      if (sym < 16) {
        hs->lens[i] = (uint8_t)sym;  // every lane stores the same byte: no exec-mask change on the scalar path
        prev = sym;
        i++;
      } else {
        const uint32_t nb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
        if (sym == 16 && i == 0) return MD_INVALID_DICTIONARY;
        ub.fill();
        if (CHECK && (int32_t)(tot - ub.pos()) < (int32_t)nb) return MD_UNEXPECTED_END_OF_INPUT;
        const uint32_t copy = ub.peekb(nb) + (sym == 18 ? 11 : 3);
        ub.drop(nb);
        const uint32_t val = sym == 16 ? prev : 0;
        if (i + copy > max_res) return MD_INVALID_DICTIONARY;
        if (val)
          for (uint32_t x = lane; x < copy; x += kWave) hs->lens[i + x] = (uint8_t)val;
        prev = val;
        i += copy;
      }
    }
    return MD_OK;
  };
  {
    const bool plenty = (int32_t)(tot - ub.pos()) >= 316 * 14 + 64;
    const int rc = plenty ? run_lengths(std::false_type{}) : run_lengths(std::true_type{});
    if (rc != MD_OK) return rc;
  }
  *bp_out = ub.pos();
  pf.tick_lds(P_HDR_LENS);
  if (uni(hs->lens[256]) == 0) return MD_INVALID_DICTIONARY;
  // the two alphabets, lane-parallel
  uint32_t ll[5], dl[1];
#pragma unroll
  for (int k = 0; k < 5; k++) ll[k] = lane + 64 * k < hlit ? (uint32_t)hs->lens[lane + 64 * k] : 0u;
  dl[0] = lane < hdist ? (uint32_t)hs->lens[hlit + lane] : 0u;
  Canon cl_, cd_;
  canon_counts<5>(ll, 9, cl_);
  canon_counts<1>(dl, 6, cd_);
  // De.Inf.huffman's verdicts (lib/de.ml:549-550): over-subscribed, or incomplete unless the longest code is 1 bit
  if (cl_.left == 0xffffffffu || (cl_.left > 0 && cl_.max != 1)) return MD_INVALID_DICTIONARY;
  const uint32_t lroot = cl_.root;
  uint32_t droot;
  lds_u32 *lut = (lds_u32 *)sm->lut;
  if (cd_.max == 0) {
    droot = 1;
  } else {
    if (cd_.left == 0xffffffffu || (cd_.left > 0 && cd_.max != 1)) return MD_INVALID_DICTIONARY;
    droot = cd_.root;
  }
  if (!build_walk<5>(ll, cl_, lut, kLitB, kLitSubB, kLitSize, hs, lane, e_root(lroot),
                     [=](uint32_t sym, uint32_t codelen) { return lit_leaf(sym, codelen, lroot, droot); }))
    return MD_INVALID_DICTIONARY;
  pf.tick_lds(P_HDR_LIT);
  if (cd_.max == 0) {  // empty_table: symbol 0 on a 1-bit code, the other slot is an error (D2)
    if (lane == 0) {
      lut[kDistB] = dist_leaf(0, 1, lroot);
      lut[kDistB + 1] = mk_entry(0, 0, 0, 0, kStopBadI);
    }
  } else if (!build_walk<1>(dl, cd_, lut, kDistB, kDistB + (1u << droot), kDistSize, hs, lane, e_root(lroot),
                            [=](uint32_t sym, uint32_t codelen) { return dist_leaf(sym, codelen, lroot); }))
    return MD_INVALID_DICTIONARY;
  const bool loopy = cl_.left > 0 || (cd_.max != 0 && cd_.left > 0);
  *lroot_out = lroot | (loopy ? kLoopy : 0u);
  return MD_OK;
}

// fixed_lit / fixed_dist (lib/de.ml:821-833): 288 lit/len codes of 8/9/7/8 bits, 32 distance codes of 5 bits
__device__ __noinline__ void fixed_tables(lds_smem *sm, uint32_t lane, uint32_t *lroot_out) {
  lds_hscratch *hs = hscratch_of(sm);
  uint32_t ll[5], dl[1];
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const uint32_t n = lane + 64 * k;
    ll[k] = n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : n < 288 ? 8 : 0;
  }
  dl[0] = lane < 32 ? 5 : 0;
  Canon cl_, cd_;
  canon_counts<5>(ll, 9, cl_);
  canon_counts<1>(dl, 6, cd_);
  const uint32_t lroot = cl_.root, droot = cd_.root;
  lds_u32 *lut = (lds_u32 *)sm->lut;
  build_walk<5>(ll, cl_, lut, kLitB, kLitSubB, kLitSize, hs, lane, e_root(lroot),
                [=](uint32_t sym, uint32_t codelen) { return lit_leaf(sym, codelen, lroot, droot); });
  build_walk<1>(dl, cd_, lut, kDistB, kDistB + (1u << droot), kDistSize, hs, lane, e_root(lroot),
                [=](uint32_t sym, uint32_t codelen) { return dist_leaf(sym, codelen, lroot); });
  *lroot_out = lroot;
}

// ---- the walks ----------------------------------------------------------------------------------
// A lane's bit cursor: two consecutive window words in registers and the one after them on its way (fetched a step
// ahead), so the only LDS access a step waits for is its table entry.
struct Cursor {
  uint32_t w0, w1, w2, wa;  // window words at byte address wa, wa + 4, wa + 8
  __device__ __forceinline__ void init(const lds_u32 *win, uint32_t p) {
    wa = (p >> 5) << 2;
    const lds_u32 *q = reinterpret_cast<const lds_u32 *>(reinterpret_cast<const lds_u8 *>(win) + wa);
    w0 = q[0];
    w1 = q[1];
    w2 = q[2];
  }
  __device__ __forceinline__ uint32_t peek(uint32_t p) const { return __builtin_amdgcn_alignbit(w1, w0, p); }  // (uses p & 31)
  __device__ __forceinline__ void seek(const lds_u32 *win, uint32_t pn) {  // pn at most one word further on
    const uint32_t wan = (pn >> 5) << 2;
    const bool ge = wan != wa;
    w0 = ge ? w1 : w0;
    w1 = ge ? w2 : w1;
    wa = wan;
    w2 = *reinterpret_cast<const lds_u32 *>(reinterpret_cast<const lds_u8 *>(win) + wa + 8);
  }
};
// the table entry the step in state `e` (the entry of the step before) finds at the bits w
__device__ __forceinline__ uint32_t lut_step(const lds_u32 *lut, uint32_t e, uint32_t w) {
  return lut_at(lut, e >> 21, __builtin_amdgcn_ubfe(w, 0, e >> 17));  // (v_bfe_u32 takes the low 5 bits of the width: the next index width)
}

// One token-boundary walk of this lane's zone [start, limit).  COUNT adds what the tokens produce: a byte per return
// to the lit/len root (a literal, or the last byte of a match), length - 1 and a match at every length code.
// A divergent per-lane loop: finished lanes leave the exec mask, the wave leaves when it is empty.  The walk goes on
// while `key` < `thr` (see the table layout); every step of a complete code consumes a bit, so it ends.  BUDGET: the
// block has an incomplete code (allowed when the only code is 1 bit long, lib/de.ml:549-550), whose unused slot
// consumes nothing (lib/de.ml:521: a zero entry is "0 bits, symbol 0"): the walk is then limited to KMAX steps.
// MID (counting passes): also the first token boundary at or beyond `mthr` (the middle of the zone) and what the tokens
// before it produce - where the zone is cut when the stream's two wavefronts emit it together (0xffffffff: none, the zone's
// tokens end before the middle or the walk stopped there).
template <bool COUNT, bool BUDGET, bool MID = false>
__device__ __forceinline__ void sync_pass(const lds_u32 *win, const lds_u32 *lut, uint32_t lroot, bool go, uint32_t start,
                                          uint32_t limit, uint32_t &end, uint32_t &stop, uint32_t &nb, uint32_t mthr = 0,
                                          uint32_t *midp = nullptr, uint32_t *midcnt = nullptr) {
  if (go) {
    uint32_t p = start, e = e_root(lroot), cnt = 0;
    uint32_t mp = 0xffffffffu, mc = 0;
    bool got = false;
    if (MID && start >= mthr) {  // (the token before reached beyond the middle: everything is the second half's)
      mp = start;
      got = true;
    }
    if (p < limit) {
      const uint32_t thr = (kLitB << 21) | limit;
      uint32_t slot = 0, key;
      Cursor c;
      c.init(win, start);
      do {
        const uint32_t w = c.peek(p);
        const uint32_t en = lut_step(lut, e, w);
        const uint32_t n = e_n(en);
        if (COUNT) {  // bytes in the low 20 bits, matches above (kCountMatch)
          const uint32_t xb = e_xb(en);
          const uint32_t len1 = e_val(en) + __builtin_amdgcn_ubfe(w, n - xb, xb) + (kCountMatch + 2);  // length - 1, and a match
          cnt += (e_tb(en) == kLitB ? 1u : 0u) + (e_tb(en) == kDistB ? len1 : 0u);
        }
        p += n;
        if (MID) {
          const bool cross = (e_tb(en) == kLitB) & !got & (p >= mthr);
          mp = cross ? p : mp;
          mc = cross ? cnt : mc;
          got = got | cross;
        }
        c.seek(win, p);
        e = en;
        key = (en & kTbMask) | p;
        if (BUDGET && ++slot >= KMAX && e_tb(en) == kLitB) break;
      } while (key < thr);
    }
    end = p;
    stop = e_tb(e) >= kStopEobI ? e_tb(e) : 0u;
    if (COUNT) nb = cnt;
    if (MID) {
      *midp = mp;
      *midcnt = mc;
    }
  }
}

struct LaneOut {
  uint32_t endp;   // bit after the last token taken (a token boundary)
  uint32_t stopc;  // 0 = zone done, kStEob, kStTrunc (round capacity), else MD_* status of the failing token
  uint32_t bytes;  // bytes produced (up to the failing token)
  uint32_t nm;     // match records written (from the lane's first record on)
};

// The token at ptok, with every check in the oracle's order (oracle/de_inflate.c ns_inflate_block): called for
// the lanes the emit pass stopped.  Returns the stop reason (< 256) | the bit after an end-of-block code << 8 - in ONE
// value: as an out-parameter of this call the caller's variable lived in scratch memory, a store and a load of every
// emit pass whether anything had stopped or not.
__device__ __noinline__ uint32_t slow_token(const lds_u32 *win, const lds_u32 *lut, uint32_t lroot, uint32_t ptok, uint32_t q,
                                            uint32_t tot, uint32_t cap) {
  uint32_t p = ptok;
  uint32_t w = peek(win, p);
  uint32_t e = lut_step(lut, e_root(lroot), w);
  if (e_link(e)) {
    p += e_n(e);
    w = peek(win, p);
    e = lut_step(lut, e, w);
  }
  uint32_t n = e_n(e), xb = e_xb(e), ntb = e_tb(e);
  uint32_t pn = p + n;
  if (pn > tot) return MD_UNEXPECTED_END_OF_INPUT;  // D1
  if (ntb == kStopEobI) return kStEob | (pn << 8);
  if (ntb != kDistB) {  // literal
    if (q >= cap) return MD_UNEXPECTED_END_OF_OUTPUT;
    return kStTrunc;
  }
  const uint32_t mlen = e_val(e) + 3 + __builtin_amdgcn_ubfe(w, n - xb, xb);
  p = pn;
  w = peek(win, p);
  e = lut_step(lut, e, w);
  if (e_tb(e) == kStopBadI && e_n(e) == 0) return MD_INVALID_DISTANCE_CODE;  // D2: an empty slot
  if (e_link(e)) {
    p += e_n(e);
    w = peek(win, p);
    e = lut_step(lut, e, w);
  }
  n = e_n(e), xb = e_xb(e);
  pn = p + n;
  if (pn > tot) return MD_UNEXPECTED_END_OF_INPUT;
  if (e_tb(e) == kStopBadI) return MD_INVALID_DISTANCE_CODE;  // the symbols 30 and 31
  const uint32_t d = dist_value(e_val(e), xb, __builtin_amdgcn_ubfe(w, n - xb, xb));
  const uint32_t lim = q < 32768u ? q : 32768u;
  if (d > lim) return MD_INVALID_DISTANCE;
  if (mlen > cap - q) return MD_UNEXPECTED_END_OF_OUTPUT;
  return kStTrunc;  // the token is fine: the round's staging buffer is full
}

// The emit pass: the same walk from a validated start, producing output.  Straight-line per step; anything
// unusual stops the lane in front of the token (ptok) and is classified afterwards by slow_token.  CHECKED = false
// leaves out the tests the caller has ruled out for the whole round: the end of the input is beyond the window, the
// output position is past 32 KiB (no distance can reach before the start) and everything counted fits the staging
// buffer and the output capacity; the only stops left are the STOP entries, which end the loop like the zone's end
// does.  A length code leaves the match length in mlen until its distance code returns to the root: a step that
// returns to the root with mlen == 0 is a literal.
template <bool CHECKED, bool BUDGET>
__device__ __forceinline__ void emit_pass(const lds_u32 *win, const lds_u32 *lut, uint32_t lroot, lds_u32 *mrec,
                                          lds_u16 *mpos, lds_u8 *stage, uint32_t rec0, uint32_t tot, bool go, uint32_t start,
                                          uint32_t limit, uint32_t q0, uint32_t rb, uint32_t R0, uint32_t cap, LaneOut &lo) {
  // rec0 = the lane's first record: the walk before counted the matches, the lanes' records follow each other
  uint32_t p = start, ptok = start, e = e_root(lroot);
  uint32_t q = q0, rec = rec0, mlen = 0;
  bool stopped = false;
  const uint32_t qlim = rb + STAGE - 16;  // the staging buffer holds output positions [rb, qlim)
  const uint32_t qmax = cap < qlim ? cap : qlim;
  if (go && p < limit) {
    const uint32_t thr = (kLitB << 21) | limit;
    uint32_t slot = 0, key;
    Cursor c;
    c.init(win, start);
    do {
      const uint32_t w = c.peek(p);
      const uint32_t en = lut_step(lut, e, w);
      const uint32_t n = e_n(en), xb = e_xb(en), ntb = e_tb(en);
      const uint32_t x = __builtin_amdgcn_ubfe(w, n - xb, xb);
      const uint32_t pn = p + n;
      const bool to_root = ntb == kLitB, is_len = ntb == kDistB;
      const bool mat = to_root & (mlen != 0), lit = to_root & (mlen == 0);
      const uint32_t d1 = (e_val(en) << xb) + x;  // distance - 1 (when this is the distance step)
      if (CHECKED) {
        const uint32_t lim = q < 32768u ? q : 32768u;
        const uint32_t need = mat ? mlen : 1u;
        stopped = (ntb >= kStopEobI) | (pn > tot) | (mat & (d1 >= lim)) | (to_root & (q + need > qmax));
        if (stopped) break;
      }
      stage[lit ? q - rb : STAGE + 15] = (uint8_t)(en >> 9);  // (a slack byte when the step is not a literal: no branch)
      if (mat) {
        mrec[rec] = ((mlen - 3) << 16) | ((q - d1 + mlen > R0 + 1) ? kNearBit : 0u) | d1;
        mpos[rec] = (uint16_t)(q - rb);
        rec++;
      }
      q += to_root ? (mlen > 1u ? mlen : 1u) : 0u;
      mlen = is_len ? e_val(en) + 3 + x : to_root ? 0u : mlen;
      p = pn;
      ptok = to_root ? pn : ptok;  // the start of the token the next step belongs to
      c.seek(win, p);
      e = en;
      key = (en & kTbMask) | p;
      if (BUDGET && ++slot >= KMAX && to_root) break;
    } while (key < thr);
    // (unchecked: the walk has gone through the code that leads to a STOP entry - an end-of-block code or an invalid
    // distance symbol; nothing was written for that token, which began at ptok)
    if (!CHECKED) stopped = e_tb(e) >= kStopEobI;
  }
  uint32_t stopc = 0, endp = p;
  if (go && stopped) {
    const uint32_t r = slow_token(win, lut, lroot, ptok, q, tot, cap);
    stopc = r & 0xffu;
    endp = stopc == kStEob ? r >> 8 : ptok;
  }
  if (go) {
    lo.endp = endp;
    lo.stopc = stopc;
    lo.bytes = q - q0;
    lo.nm = rec - rec0;
  }
}

// ---- a round's sync passes and its verdict ----------------------------------------------------------
// What the sync passes of a round leave: per lane the validated start of its zone, where its walk ended, the STOP table it
// ran into (0: none), what its tokens produce (bytes | matches << 20) and whether that was counted from the validated
// start; wave-uniform the consistent prefix of lanes and the passes walked.  MID: the cut in the zone's middle and what
// lies before it (sync_pass).
struct SyncRound {
  uint32_t start, end, stop, nb, limit;
  bool counted;
  uint32_t nvalid, np;
  uint32_t midp, midcnt;
};
// the lanes whose chain start_i == end_{i-1} holds from lane 0 on (lane 0 is always counted: >= 1)
__device__ __forceinline__ uint32_t consistent_prefix(const SyncRound &r, uint32_t lane) {
  const uint32_t pe = wave_shr1(r.end), ps = wave_shr1(r.stop);
  const uint64_t bad = __ballot(!r.counted || (lane > 0 && (ps != 0 || pe != r.start)));
  return bad ? (uint32_t)__builtin_ctzll(bad) : 64;
}
// 64 zones of zs bits from window bit rbp on: the speculative pass, the counting passes, the consistent prefix.  pf gets
// the time of the first pass and a count per pass.
template <bool BUDGET, bool MID, class PF>
__device__ __forceinline__ SyncRound sync_round(const lds_u32 *win, const lds_u32 *lut, uint32_t lroot, uint32_t lane, uint32_t rbp,
                                                uint32_t zs, PF &pf) {
  SyncRound r;
  r.start = rbp + lane * zs, r.end = 0, r.stop = 0, r.nb = 0;
  r.midp = 0xffffffffu, r.midcnt = 0;
  r.limit = rbp + (lane + 1) * zs;
  // the speculative pass starts a RUN-IN ahead of the zone (inside the zone before): all it has to deliver is the
  // boundary at the zone's END, and the longer the walk, the likelier that it has synchronised by then - fewer lanes
  // walk again in passes 2+, which cost a full pass each for a handful of lanes (the pass without counts is the
  // cheap one: 24 instructions a step against 34)
  const uint32_t runin_ = (zs * RUNIN_NUM) / RUNIN_DEN, runin = runin_ < lane * zs ? runin_ : lane * zs;  // (not before the round's start)
  r.counted = false;
  pf.count(C_PASSES);
  sync_pass<false, BUDGET>(win, lut, lroot, true, r.start - runin, r.limit, r.end, r.stop, r.nb);
  pf.tick(P_DECODE1);
  r.np = 1;
  const uint32_t passes = zs * PASSES >= PASS_BITS ? PASSES : PASS_BITS / zs > PASSES_MAX ? PASSES_MAX : PASS_BITS / zs;
#pragma nounroll  // (with a constant zone size `passes` is a constant: one copy of the counting walk, not six)
  for (uint32_t it = 0; it < passes; it++) {
    const uint32_t pe = wave_shr1(r.end), ps = wave_shr1(r.stop);
    const bool redo = lane == 0 ? !r.counted : (ps == 0 && (pe != r.start || !r.counted));
    if (__ballot(redo) == 0) break;
    if (redo && lane > 0) r.start = pe;
    pf.count(C_PASSES);
    r.np++;
    if constexpr (MID) sync_pass<true, BUDGET, true>(win, lut, lroot, redo, r.start, r.limit, r.end, r.stop, r.nb, r.limit - (zs * MD_SPLIT_B) / 8, &r.midp, &r.midcnt);
    else sync_pass<true, BUDGET>(win, lut, lroot, redo, r.start, r.limit, r.end, r.stop, r.nb);
    r.counted = r.counted || redo;
  }
  r.nvalid = consistent_prefix(r, lane);
  return r;
}

// How a round ends.  The first stopped lane (stream order) ends it: its reason, the bytes and records in front of its
// failing token, and the lanes behind it are void; with no lane stopped, what the nvalid lanes produce together (all_*).
// boff / roff: the bytes / records of the lanes before this one.
struct Verdict {
  uint32_t lstop, nvalid, total, nrec;
};
__device__ __forceinline__ Verdict round_verdict(bool mine, const LaneOut &lo, uint32_t boff, uint32_t roff, uint32_t nvalid,
                                                 uint32_t all_bytes, uint32_t all_rec) {
  Verdict v = {0, nvalid, all_bytes, all_rec};
  const uint64_t fm = __ballot(mine && lo.stopc != 0);
  if (fm) {
    const uint32_t fl = __builtin_ctzll(fm);
    v.lstop = rdlane(lo.stopc, fl);
    v.total = rdlane(boff, fl) + rdlane(lo.bytes, fl);
    v.nrec = rdlane(roff, fl) + rdlane(lo.nm, fl);  // later lanes are void
    v.nvalid = fl + 1;
  }
  return v;
}

// ---- a stream from its first byte to its last block ---------------------------------------------------
// What both kernels do first with a stream's descriptor: an input that 32-bit bit positions cannot address is refused
// (rc = MD_E_INVALID_ARGUMENT: the descriptor is out of range, mdeflate.h; what is written then is the kernel's own), and
// the zlib frame comes off (Zl.Inf.Ns.inflate, lib/zl.ml:400-417).  The DEFLATE body is src[body_off, body_off + body_len).
struct Opened {
  int rc;
  uint32_t body_off, body_len;
};
__device__ __forceinline__ Opened open_stream(int format, const uint8_t *src, uint64_t slen64) {
  Opened o = {MD_OK, 0, (uint32_t)slen64};
  if (slen64 > MD_MAX_INFLATE_IN) {
    o.rc = MD_E_INVALID_ARGUMENT;
  } else if (format == MD_FORMAT_ZLIB) {
    const uint32_t slen = (uint32_t)slen64;
    if (slen < 2) o.rc = MD_UNEXPECTED_END_OF_INPUT;
    else {
      uint32_t cmf = src[0], flg = src[1];
      if (((cmf << 8) + flg) % 31 != 0 || (cmf & 0xf) != 8) o.rc = MD_INVALID_HEADER;
      else if (slen < 6) o.rc = MD_UNEXPECTED_END_OF_INPUT;
      else {
        o.body_off = 2;
        o.body_len = slen - 6;
      }
    }
  }
  return o;
}

// A block header that still lies within this many bits of the window in LDS is read from there.  A stored block's LEN/NLEN
// word is only ever met behind such a header (window bit <= kHeaderReuse + 3), so it lies in the window too:
constexpr uint32_t kHeaderReuse = 4096;
static_assert((kHeaderReuse + 3 + 7) / 8 + 4 <= (WIN_WORDS - 2) * 4, "a stored block's LEN/NLEN is read from the window in LDS");

// All blocks of a body, from bit bp on: the block headers, the runs of empty fixed blocks, the stored headers, the table
// builders; the status is that of the first failing check, in the reference's order.  The handler H has what differs between
// the decoder and the size query:
//   int stored(p, len)             the payload body[p, p + len) of a stored block (len may be 0)
//   void fixed(&lroot)             fixed_tables: the root width
//   int dynamic(rbp, tot, &hend, &lroot)   dynamic_tables: the window bit behind the header, the root width (| kLoopy)
//   void header_done()             the tables are built (a profile tick)
//   int huffman<BUDGET>(lroot, &bp)  all rounds of the Huffman block
//   void block_done(&rc, bp, last)   a block is complete
template <class H>
__device__ __forceinline__ int block_loop(H &h, lds_smem *sm, const uint8_t *__restrict__ body, uint32_t body_len, uint32_t lane,
                                          uint32_t &bp, Window &wnd) {
  lds_u32 *win = (lds_u32 *)sm->win;
  const uint32_t total_bits = body_len * 8;
  int rc = MD_OK;
  bool last = false;
  uint32_t fixed_lroot = 0;         // != 0: the tables in LDS are the fixed ones (and this is their root width)
  uint32_t lds_base = 0xffffffffu;  // the window in LDS begins at this byte of the body (nothing else has been loaded since)
  while (!last && rc == MD_OK) {
    // a block header that still lies in the first part of the window in LDS is read from there: runs of tiny blocks
    // (flush points, empty blocks) would otherwise load 2 KiB from the input for every few bytes of it
    uint32_t base = (bp >> 5) << 2;
    if (lds_base != 0xffffffffu && bp >= lds_base * 8 && bp - lds_base * 8 <= kHeaderReuse) base = lds_base;
    else {
      wnd.ensure(win, body, body_len, base, lane);
      lds_base = base;
    }
    uint32_t rbp = bp - base * 8;
    const uint32_t tot = total_bits - base * 8;
    if ((int32_t)(tot - rbp) < 3) {
      rc = MD_UNEXPECTED_END_OF_INPUT;
      break;
    }
    const uint32_t hdr = uni(peek(win, rbp));
    last = hdr & 1;
    const uint32_t type = (hdr >> 1) & 3;
    bp += 3;
    rbp += 3;
    bool block_done = false;  // the block was dealt with here (an empty fixed one)
    if (type == 1) {
      // a run of EMPTY fixed blocks - header, then the 7-bit end-of-block code 0000000 (lib/de.ml:821-833) - is walked
      // through right here: ten bits a block instead of a round each
      for (;;) {
        if (rbp + 7 > tot || rbp + 64 > WIN_WORDS * 32 - 64 || (uni(peek(win, rbp)) & 0x7fu) != 0) break;  // not one of them
        rbp += 7;
        bp += 7;
        block_done = true;  // the block whose header was consumed last is complete
        if (last || rbp + 3 > tot) break;
        const uint32_t h3 = uni(peek(win, rbp)) & 7u;
        if (((h3 >> 1) & 3) != 1) break;  // another kind of block: back to the loop above
        last = h3 & 1;
        rbp += 3;
        bp += 3;
        block_done = false;
      }
    }
    if (block_done) {
      // nothing to decode
    } else if (type == 0) {
      // flat, lib/de.ml:1613-1627
      uint32_t p = (bp + 7) >> 3;
      if (body_len - p < 4) {
        rc = MD_UNEXPECTED_END_OF_INPUT;
        break;
      }
      const uint32_t h4 = uni(peek(win, (p - base) * 8));
      const uint32_t len = h4 & 0xffff, nlen = h4 >> 16;
      p += 4;
      if (nlen != 0xffff - len) rc = MD_INVALID_COMPLEMENT_OF_LENGTH;
      else if (len > body_len - p) rc = MD_UNEXPECTED_END_OF_INPUT;
      else {
        rc = h.stored(p, len);
        if (rc == MD_OK) bp = (p + len) * 8;
      }
    } else if (type == 3) {
      rc = MD_INVALID_KIND_OF_BLOCK;
    } else {
      uint32_t lroot = 0;
      if (type == 1) {
        if (fixed_lroot == 0) {  // (a run of fixed blocks builds their tables once)
          h.fixed(lroot);
          fixed_lroot = uni(lroot);
        }
        lroot = fixed_lroot;
      } else {
        uint32_t hend = 0;
        fixed_lroot = 0;
        rc = h.dynamic(rbp, tot, hend, lroot);
        bp = base * 8 + hend;
      }
      lroot = uni(lroot);
      h.header_done();
      if (rc == MD_OK) {
        if (lroot & kLoopy) rc = h.template huffman<true>(lroot & 15, bp);
        else rc = h.template huffman<false>(lroot, bp);
        lds_base = 0xffffffffu;
      }
    }
    h.block_done(rc, bp, last);
  }
  return rc;
}

}  // namespace wv
}  // namespace md
