// inflate_count.hip — the size query of the batch decoder for gfx950 (md_inflate_sizes_batch_*, md_inflate_plan_device):
// every stream's inflated size without decoding it, the GZIP trailer check that goes with it, and the output plan.
#include <stddef.h>
// The decoder's record pool and staging buffer shape only the tail of Smem, which nothing in this file touches (see
// CountSmem); the values are the decoder's so that the shared header's checks of them hold.
#define MD_RMAX 576
#define MD_STAGE 5248
#include "inflate_wave_core.hpp"

namespace md {
namespace wv {

// ---- the size query: md_inflate_sizes_batch_* ----------------------------------------------------
// inflate_count_kernel walks a stream like the decoder and produces nothing: one wavefront per stream, no copier, no
// staging buffer, no records, no checksum.  The stream's opening and its block loop are the decoder's (open_stream,
// block_loop in inflate_wave_core.hpp; CountBlocks below is this kernel's side of it), and so is a round: 64 zones of S
// bits through sync_round - the speculative pass, the counting passes and the consistent prefix of lanes.  Then
//   plain    (the input ends beyond the window, the output position is past 32 KiB, no accepted lane ran into a STOP
//            entry) nothing else can fail: the lanes' byte counts are summed and the round is over - no second walk;
//   checked  (the first 32 KiB of output, the tail of the input, a STOP entry) one walk over the accepted lanes with
//            emit_pass<true>'s tests and none of its stores; a stopped lane's token is classified by slow_token with a
//            capacity that is never reached, the first stopped lane in stream order decides.
// The position is 64-bit (a size beyond MD_MAX_STREAM is a result, not an error); what the distance rule needs of it
// saturates at 32 768.  A round is not bounded by a staging buffer, so its bytes do not fit the packed count's low 20
// bits once summed (64 lanes x 132 two-bit matches x 258 bytes): the byte field is summed on its own, per lane it fits.
// The shared device functions take the decoder's Smem and touch only its first two members, the window (with the
// header scratch in its tail) and the walk table: CountSmem is that prefix.
struct CountSmem {
  uint32_t win[WIN_WORDS];
  uint32_t lut[kLutWords];
  uint32_t hout[2];  // what fixed_tables / dynamic_tables hand back (root width, header end): here, the kernel keeps no stack slots for them
};
static_assert(offsetof(Smem, win) == offsetof(CountSmem, win) && offsetof(Smem, lut) == offsetof(CountSmem, lut),
              "dynamic_tables / fixed_tables address the window and the table through an Smem pointer");
static_assert(sizeof(CountSmem) <= 8192, "20 streams (20 wavefronts) per CU: 160 KiB / 20");
constexpr uint32_t kStUnbounded = 102;  // lane stop reason of count_block only: the stream stands still and produces output
struct CountProf {  // the count kernel's profile: dbg[0..2], summed over the batch
  uint32_t rounds, passes, checked;
};
// (dynamic_tables takes a profile by reference: a global one costs the kernel no stack slot)
__device__ Prof<false> g_count_pf;

// emit_pass<true, BUDGET> without its stores and without an output or staging limit: q counts this lane's bytes, qs is
// the (saturated) output position the lane begins at
template <bool BUDGET>
__device__ __forceinline__ void check_pass(const lds_u32 *win, const lds_u32 *lut, uint32_t lroot, uint32_t tot, bool go,
                                           uint32_t start, uint32_t limit, uint32_t qs, LaneOut &lo) {
  uint32_t p = start, ptok = start, e = e_root(lroot);
  uint32_t q = 0, mlen = 0;
  bool stopped = false;
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
      const bool mat = to_root & (mlen != 0);
      const uint32_t d1 = (e_val(en) << xb) + x;  // distance - 1 (when this is the distance step)
      const uint32_t at = qs + q, lim = at < 32768u ? at : 32768u;
      stopped = (ntb >= kStopEobI) | (pn > tot) | (mat & (d1 >= lim));
      if (stopped) break;
      q += to_root ? (mlen > 1u ? mlen : 1u) : 0u;
      mlen = is_len ? e_val(en) + 3 + x : to_root ? 0u : mlen;
      p = pn;
      ptok = to_root ? pn : ptok;
      c.seek(win, p);
      e = en;
      key = (en & kTbMask) | p;
      if (BUDGET && ++slot >= KMAX && to_root) break;
    } while (key < thr);
  }
  uint32_t stopc = 0, endp = p;
  if (go && stopped) {
    const uint32_t r = slow_token(win, lut, lroot, ptok, qs + q, tot, 0xffffffffu);
    stopc = r & 0xffu;
    endp = stopc == kStEob ? r >> 8 : ptok;
  }
  if (go) {
    lo.endp = endp;
    lo.stopc = stopc;
    lo.bytes = q;
    lo.nm = 0;
  }
}

// All rounds of one Huffman block, counted.  On return *bp_io is the bit after the EOB and pos has grown by the block's
// bytes (on a failure: by the bytes in front of the failing token).
template <bool BUDGET>
__device__ __forceinline__ int count_block(lds_smem *sm, const uint8_t *__restrict__ body, uint32_t body_len, uint64_t &pos,
                                           uint32_t lroot, uint32_t lane, uint32_t *bp_io, Window &wnd, CountProf &cc) {
  uint32_t bp = *bp_io;
  lds_u32 *win = (lds_u32 *)sm->win;
  const lds_u32 *lut = (const lds_u32 *)sm->lut;
  const uint32_t total_bits = body_len * 8;
  for (;;) {
    const uint32_t base = (bp >> 5) << 2;
    wnd.ensure(win, body, body_len, base, lane);
    const uint32_t rbp = bp - base * 8, tot = total_bits - base * 8;  // window-relative
    const SyncRound r = sync_round<BUDGET, false>(win, lut, lroot, lane, rbp, S, g_count_pf);  // (S: passes and run-in are constants)
    const bool mine = lane < r.nvalid;
    const uint32_t mybytes = mine ? r.nb & (kCountMatch - 1) : 0u;  // (a lane's own count fits; the matches are not needed)
    const bool plain = tot >= rbp + kWave * S + 64 && pos >= 32768u && rdlane(r.stop, r.nvalid - 1) == 0;
    uint32_t total, lstop = 0, nbp;
    if (plain) {
      total = wave_sum(mybytes);
      nbp = base * 8 + rdlane(r.end, r.nvalid - 1);
    } else {
      const uint32_t boff = wave_excl_scan(mybytes, lane);
      const uint32_t ps32 = pos < 32768u ? (uint32_t)pos : 32768u;
      LaneOut lo;
      lo.endp = r.end, lo.stopc = 0, lo.bytes = 0, lo.nm = 0;
      check_pass<BUDGET>(win, lut, lroot, tot, mine, r.start, r.limit, ps32 + boff < 32768u ? ps32 + boff : 32768u, lo);
      const Verdict v = round_verdict(mine, lo, boff, 0, r.nvalid, wave_sum(mine ? lo.bytes : 0u), 0);
      lstop = v.lstop;
      total = v.total;
      nbp = base * 8 + rdlane(lo.endp, v.nvalid - 1);
    }
    cc.rounds++;  // (wave-uniform: three scalar additions a round)
    cc.passes += r.np;
    cc.checked += plain ? 0u : 1u;
    wnd.fetch(body, body_len, (nbp >> 5) << 2, lane);  // the next round's (or the next block header's) window: on its way
    if (nbp == bp && (lstop == 0 || lstop == kStTrunc)) {
      // No bit consumed.  With output: an incomplete one-code block stands on its unused slot, which the reference reads as
      // a literal of no bits - the output never ends.  Without: defensive, as in inflate_block.
      return total && BUDGET ? (int)kStUnbounded : MD_E_HIP;
    }
    pos += total;
    bp = nbp;
    if (lstop == kStEob) break;
    if (lstop == kStTrunc) return MD_E_HIP;  // (slow_token found nothing wrong with a token the walk stopped at)
    if (lstop != 0) return (int)lstop;
  }
  *bp_io = bp;
  return MD_OK;
}

// The size query's side of block_loop (inflate_wave_core.hpp): a stored block is arithmetic, a Huffman block is counted.
struct CountBlocks {
  lds_smem *sm;
  MD_LDS uint32_t *hout;  // CountSmem::hout
  const uint8_t *body;
  uint32_t body_len, lane;
  Window &wnd;
  uint64_t pos;  // bytes so far
  CountProf cc;
  __device__ __forceinline__ int stored(uint32_t, uint32_t len) {
    pos += len;
    return MD_OK;
  }
  __device__ __forceinline__ void fixed(uint32_t &lroot) {
    fixed_tables(sm, lane, (uint32_t *)&hout[0]);
    lroot = hout[0];
  }
  __device__ __forceinline__ int dynamic(uint32_t rbp, uint32_t tot, uint32_t &hend, uint32_t &lroot) {
    const int rc = dynamic_tables(sm, rbp, tot, lane, (uint32_t *)&hout[1], (uint32_t *)&hout[0], g_count_pf);
    if (rc == MD_OK) {
      lroot = hout[0];
      hend = uni(hout[1]);
    }
    return rc;
  }
  __device__ __forceinline__ void header_done() {}
  template <bool BUDGET>
  __device__ __forceinline__ int huffman(uint32_t lroot, uint32_t &bp) {
    return count_block<BUDGET>(sm, body, body_len, pos, lroot, lane, &bp, wnd, cc);
  }
  __device__ __forceinline__ void block_done(int &, uint32_t, bool) {}
};

template <bool PROF>
__global__ __launch_bounds__(kWave, 5) void inflate_count_kernel(int format, uint32_t n, const uint8_t *__restrict__ in,
                                                                 const uint64_t *__restrict__ in_off,
                                                                 const uint64_t *__restrict__ in_len,
                                                                 uint64_t *__restrict__ out_len, uint64_t *__restrict__ consumed,
                                                                 int32_t *__restrict__ status, uint64_t *__restrict__ dbg,
                                                                 const uint32_t *__restrict__ order) {
  __shared__ CountSmem smem;
  lds_smem *sm = (lds_smem *)&smem;  // (its window and table only: see CountSmem)
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x >= n) return;
  const uint32_t sid = order ? order[blockIdx.x] : blockIdx.x;
  const uint8_t *src = in + in_off[sid];
  const Opened o = open_stream(format, src, in_len[sid]);
  if (o.rc == MD_E_INVALID_ARGUMENT) {
    if (lane == 0) {
      out_len[sid] = 0;
      consumed[sid] = 0;
      status[sid] = MD_E_INVALID_ARGUMENT;
    }
    return;
  }
  if (lane < 4) sm->lut[kStopEobI + lane] = mk_entry(0, 0, 0, 0, kStopEobI + (lane & 2));  // the self-looping STOP entries
  uint32_t bp = 0;
  Window wnd;
  wnd.base = 0xffffffffu;
  CountBlocks h = {sm, (MD_LDS uint32_t *)smem.hout, src + o.body_off, o.body_len, lane, wnd, 0, {0, 0, 0}};
  int rc = o.rc;
  if (rc == MD_OK) rc = block_loop(h, sm, h.body, h.body_len, lane, bp, wnd);
  const uint64_t pos = h.pos;
  const CountProf &cc = h.cc;
  uint32_t used = (bp + 7) >> 3;
  if (rc == MD_OK && format == MD_FORMAT_ZLIB) used += 6;  // (the Adler-32 is not compared: no byte was produced)
  if (rc == (int)kStUnbounded) rc = MD_UNEXPECTED_END_OF_OUTPUT;  // what every finite room gets
  if (lane == 0) {
    out_len[sid] = pos;
    consumed[sid] = rc == MD_OK ? used : 0;
    status[sid] = rc;
  }
  if (PROF && dbg && lane == 0) {
    atomicAdd((unsigned long long *)&dbg[0], (unsigned long long)cc.rounds);
    atomicAdd((unsigned long long *)&dbg[1], (unsigned long long)cc.passes);
    atomicAdd((unsigned long long *)&dbg[2], (unsigned long long)cc.checked);
  }
}

// GZIP after the count kernel ran on the bodies: gz_finish_kernel's order of checks without the CRC-32 (there is no
// output to sum).  One thread per stream.
__global__ __launch_bounds__(256) void sizes_gz_finish_kernel(uint32_t n, const uint8_t *__restrict__ in,
                                                              const uint64_t *__restrict__ in_off,
                                                              const uint64_t *__restrict__ in_len,
                                                              const uint64_t *__restrict__ body_off,
                                                              const int32_t *__restrict__ hstatus, uint64_t *__restrict__ out_len,
                                                              uint64_t *__restrict__ consumed, int32_t *__restrict__ status) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int hs = hstatus[i];
  int st = hs != MD_OK ? hs : status[i];
  uint64_t used = 0;
  const uint64_t wrote = hs != MD_OK ? 0 : out_len[i];
  if (st == MD_OK) {
    const uint64_t hdr = body_off[i] - in_off[i], body = consumed[i];
    if (in_len[i] - hdr - body < 8) st = MD_UNEXPECTED_END_OF_INPUT;
    else {
      const uint8_t *t = in + body_off[i] + body + 4;
      uint32_t isize = 0;
      for (int k = 0; k < 4; k++) isize |= (uint32_t)t[k] << (8 * k);
      if (isize != (uint32_t)wrote) st = MD_INVALID_SIZE;
      else used = hdr + body + 8;
    }
  }
  status[i] = st;
  consumed[i] = used;
  out_len[i] = wrote;
}

// md_inflate_plan_device: out_cap[i] = out_len[i], out_off = the exclusive sum of the caps rounded up to `align` (a power
// of two), *total = the whole.  One workgroup of 1 024, the shape of gzm::scan_kernel.
__global__ __launch_bounds__(1024) void inflate_plan_kernel(uint64_t n, const uint64_t *__restrict__ out_len, uint64_t align,
                                                            uint64_t *__restrict__ out_off, uint64_t *__restrict__ out_cap,
                                                            uint64_t *__restrict__ total) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long carry;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint64_t base = 0; base < n; base += 1024) {
    const uint64_t i = base + threadIdx.x;
    const unsigned long long len = i < n ? out_len[i] : 0;
    const unsigned long long v = (len + (align - 1)) & ~(unsigned long long)(align - 1);
    unsigned long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(x, o);
      if ((int)lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    unsigned long long before = carry;
    for (uint32_t k = 0; k < wave; k++) before += wsum[k];
    if (i < n) {
      out_off[i] = before + x - v;
      out_cap[i] = len;
    }
    __syncthreads();
    if (threadIdx.x == 1023) carry = before + x;
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = carry;
}

}  // namespace wv
}  // namespace md

// dbg != null: every stream adds its rounds, passes and checked rounds to dbg[0..2]
extern "C" int md_launch_inflate_count(int format, uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
                                       uint64_t *out_len, uint64_t *consumed, int32_t *status, uint64_t *dbg, uint32_t *order,
                                       hipStream_t stream) {
  if (n == 0) return 0;
  using namespace md::wv;
  if (order) {  // longest streams first, as the decoder
    const int e = md_launch_stream_order(n, in_len, order, stream);
    if (e != 0) return e;
  }
  if (dbg) hipLaunchKernelGGL(inflate_count_kernel<true>, dim3(n), dim3(kWave), 0, stream, format, n, in, in_off, in_len, out_len, consumed, status, dbg, order);
  else hipLaunchKernelGGL(inflate_count_kernel<false>, dim3(n), dim3(kWave), 0, stream, format, n, in, in_off, in_len, out_len, consumed, status, dbg, order);
  return (int)hipGetLastError();
}
extern "C" int md_launch_sizes_gz_finish(uint32_t n, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
                                         const uint64_t *body_off, const int32_t *hstatus, uint64_t *out_len, uint64_t *consumed,
                                         int32_t *status, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(md::wv::sizes_gz_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, in, in_off, in_len, body_off, hstatus,
                     out_len, consumed, status);
  return (int)hipGetLastError();
}
extern "C" int md_launch_inflate_plan(uint64_t n, const uint64_t *out_len, uint64_t align, uint64_t *out_off, uint64_t *out_cap,
                                      uint64_t *total, hipStream_t stream) {
  hipLaunchKernelGGL(md::wv::inflate_plan_kernel, dim3(1), dim3(1024), 0, stream, n, out_len, align, out_off, out_cap, total);
  return (int)hipGetLastError();
}
