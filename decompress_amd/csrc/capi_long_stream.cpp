// capi_long_stream.cpp — ONE long stream decoded by the whole chip (csrc/inflate_chunked.hip has the scheme and the
// kernels).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ctx.hpp"
#include "gz_frame.hpp"

// De.Higher.uncompress / Zl.Higher.uncompress / Gz on ONE big input (lib/de.ml:4555-4571, lib/zl.ml:650-666,
// bin/decompress.ml:77-100).  Returns MD_NOT_HANDLED whenever anything is not exactly as a well-formed stream decoded in
// pieces should be - the caller then takes the serial path, whose statuses and counts are the reference's; MD_OK means
// the whole stream is decoded, verified against its checksum, and copied out.
namespace {
struct ParPiece {
  uint64_t bit;      // first bit of the piece in the body (a block start)
  uint64_t u = 0;    // bytes it produces
};
}  // namespace

// What par_decode works on: a raw DEFLATE body in host memory that starts start_bit bits into body[0], the (at most 32 KiB
// of) output in front of it, room for dst_cap new bytes.  partial_ok: the body may end inside a block (a piece of a stream
// that is still arriving) - the complete blocks are decoded, the rest is the caller's.
struct ParIn {
  const uint8_t *body;
  uint64_t body_len;
  uint32_t start_bit;
  const uint8_t *hist;
  uint32_t hist_len;
  uint64_t dst_cap;
  bool partial_ok;
};
struct ParOut {
  int status;            // MD_OK: the final block ended; MD_UNEXPECTED_END_OF_INPUT (partial_ok): the body ended inside a block
  uint64_t total;        // new bytes, final, at ctx->scratch[kParOut].p + hist_len
  uint64_t used_body;    // MD_OK: bytes of the body the stream used
  uint64_t resume_bits;  // bit of the body behind the last complete block
};
// starts (may be null): the starts of pieces 1 .. of the verified chain, as ParStart states them
static int par_decode(md_ctx *ctx, const ParIn &in, ParOut *out, std::vector<ParStart> *starts = nullptr) {
  ctx->par_last_pieces = ctx->par_last_rounds = 0;
  const bool dbg_t = getenv("MD_DEBUG_HOSTPATH") != nullptr;
  const auto t_start = std::chrono::steady_clock::now();
  auto stamp = [&](const char *what) {
    if (dbg_t) fprintf(stderr, "[par_decode] %-22s at %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
  };
  const uint8_t *body = in.body;
  const uint64_t body_len = in.body_len, dst_cap = in.dst_cap;
  const uint32_t hl = in.hist_len;
  // pieces of "inflate_parallel_chunk" (64 KiB) of input - smaller ones for a smaller stream, so that it still comes in a few
  // hundred pieces (a piece is a serial decode: 880 KB of 40-byte flush units in 14 pieces took 36 ms), never under 4 KiB
  uint64_t K = ctx->par_chunk;
  if (in.body_len / 256 < K) K = (in.body_len / 256 + 4095) & ~(uint64_t)4095;
  if (K < 4096) K = 4096;
  if (body_len < 4 * K || body_len > ((uint64_t)1 << 31) || hl + dst_cap > MD_MAX_STREAM) return MD_NOT_HANDLED;
  const uint32_t nchunks = (uint32_t)((body_len + K - 1) / K);
  hipStream_t st = ctx->stream;
  // -- the body on the device, candidate block starts
  int rc = ctx->scratch[kParIn].reserve(ctx, body_len + 64, "hipMalloc(parallel inflate input)");
  if (rc != MD_OK) return rc;
  // (the slack: room for the descriptors of the rounds below, 93 bytes a row and about two rows a chunk, so that the block
  // does not grow between the rounds)
  uint64_t *d_cand = nullptr;
  rc = carve(ctx, ctx->scratch[kParDesc], "hipMalloc(parallel inflate descriptors)", [&](md::Carver &cd) {
    d_cand = cd.take<uint64_t>(nchunks - 1);
  }, (size_t)nchunks * 2 * 160 + 4096);
  if (rc != MD_OK) return rc;
  uint8_t *d_body = (uint8_t *)ctx->scratch[kParIn].p;
  HIP_TRY(ctx, hipMemcpyAsync(d_body, body, body_len, hipMemcpyHostToDevice, st));
  if (dbg_t) {
    hipStreamSynchronize(st);
    stamp("body on the device");
  }
  MD_LAUNCH_TRY(ctx, md_launch_find_blocks(d_body, body_len, K, nchunks - 1, d_cand, st));
  std::vector<uint64_t> cand(nchunks - 1);
  HIP_TRY(ctx, md::to_host(cand.data(), d_cand, cand.size(), st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  stamp("candidates found");
  // A run of STORED blocks from bit `pos` on is followed on the host, a read per block (lib/de.ml:1613-1627: header, padding,
  // LEN, NLEN): -> the bit behind the run (`pos` itself when the block there is not a stored, non-final one); *mid receives
  // block starts inside the run at least K bytes apart - stored data is the one kind whose block starts need no decoding to
  // be found, and a long run of it (incompressible input, level 0, compressed files inside a tar) should not be one piece.
  auto hop_stored = [&](uint64_t pos, std::vector<uint64_t> *mid) -> uint64_t {
    uint64_t last_mid = pos;
    for (int hops = 0; hops < (1 << 22); hops++) {
      const uint64_t by = pos >> 3;
      if (by + 5 > body_len) break;
      const uint32_t h = ((uint32_t)body[by] | ((uint32_t)body[by + 1] << 8)) >> (pos & 7);
      if ((h & 6) != 0 || (h & 1)) break;  // not stored, or the final block
      const uint64_t at = (pos + 3 + 7) >> 3;
      if (at + 4 > body_len) break;
      const uint32_t len = body[at] | ((uint32_t)body[at + 1] << 8), nlen = body[at + 2] | ((uint32_t)body[at + 3] << 8);
      if ((len ^ nlen) != 0xffffu || at + 4 + len > body_len) break;
      if (mid && pos >= last_mid + K * 8) {
        mid->push_back(pos);
        last_mid = pos;
      }
      pos = (at + 4 + len) * 8;
    }
    return pos;
  };
  std::vector<ParPiece> pc;
  pc.push_back(ParPiece{in.start_bit});
  {  // a stream that BEGINS with stored blocks: their starts are candidates the finder cannot see
    std::vector<uint64_t> mid;
    const uint64_t x = hop_stored(in.start_bit, &mid);
    if (x > in.start_bit && x < body_len * 8) mid.push_back(x);
    for (uint64_t c : mid)
      if (c > pc.back().bit) pc.push_back(ParPiece{c});
  }
  {
    const uint64_t seeded = pc.back().bit;
    for (uint64_t c : cand)
      if (c != ~0ull && c > seeded && c > pc.back().bit) pc.push_back(ParPiece{c});
  }
  if (pc.size() < 3) return MD_NOT_HANDLED;  // nothing to gain
  // -- decode, verify the chain of pieces, decode again without a candidate that proved false or with more room
  uint32_t capmul = 6;
  uint64_t total = 0, used_body = 0;
  out->status = MD_OK;
  out->resume_bits = 0;
  std::vector<uint64_t> offa, offb;
  for (int round = 1;; round++) {
    if (round > 8) return MD_NOT_HANDLED;
    ctx->par_last_rounds = round;
    const size_t np = pc.size(), n = 2 * np - 1;  // piece 0 once (its window is real), the others with window A and window B
    // out blob: [the final output: dst_cap][scratch of piece 1 A, 1 B, 2 A, ...]: 32 KiB of window + room, 64-byte aligned
    std::vector<uint64_t> in_off(n), in_len(n), out_off(n), out_cap(n);
    std::vector<uint32_t> start_bit(n), hist(n), adler_in(n, 1);
    std::vector<uint8_t> variant(n);
    offa.assign(np, 0);
    offb.assign(np, 0);
    uint64_t at = ((uint64_t)hl + dst_cap + 63) & ~(uint64_t)63;
    for (size_t p = 0; p < np; p++) {
      const uint64_t b0 = pc[p].bit >> 3, b1 = p + 1 < np ? (pc[p + 1].bit + 7) >> 3 : body_len;
      for (int v = 0; v < (p ? 2 : 1); v++) {
        const size_t i = p ? 2 * p - 1 + v : 0;
        in_off[i] = b0;
        in_len[i] = b1 - b0;
        start_bit[i] = (uint32_t)(pc[p].bit & 7);
        if (p == 0) {
          out_off[i] = 0;
          out_cap[i] = hl + dst_cap;
          hist[i] = hl;  // (the caller's window lies in front of the output)
          variant[i] = 0;
        } else {
          const uint64_t room = (uint64_t)capmul * (b1 - b0) + 65536;
          out_off[i] = at;
          out_cap[i] = 32768 + room;
          hist[i] = 32768;
          variant[i] = (uint8_t)(1 + v);
          (v ? offb : offa)[p] = at + 32768;
          at += (32768 + room + 64 + 63) & ~(uint64_t)63;
        }
      }
    }
    if (at > ((uint64_t)64 << 30)) return MD_NOT_HANDLED;
    rc = ctx->scratch[kParOut].reserve(ctx, at + 64, "hipMalloc(parallel inflate output)");
    if (rc != MD_OK) return rc;
    // the rows' descriptors, n entries each
    uint64_t *d_in_off = nullptr, *d_in_len = nullptr, *d_out_off = nullptr, *d_out_cap = nullptr, *d_out_len = nullptr, *d_consumed = nullptr,
             *d_resume_bits = nullptr, *d_resume_out = nullptr;
    uint32_t *d_start_bit = nullptr, *d_hist = nullptr, *d_adler_in = nullptr, *d_checksum = nullptr, *d_resume_adler = nullptr, *d_resume_last = nullptr;
    int32_t *d_status = nullptr;
    uint8_t *d_variant = nullptr;
    rc = carve(ctx, ctx->scratch[kParDesc], "hipMalloc(parallel inflate descriptors)", [&](md::Carver &c) {
      d_in_off = c.take<uint64_t>(n), d_in_len = c.take<uint64_t>(n), d_out_off = c.take<uint64_t>(n), d_out_cap = c.take<uint64_t>(n);
      d_out_len = c.take<uint64_t>(n), d_consumed = c.take<uint64_t>(n), d_resume_bits = c.take<uint64_t>(n), d_resume_out = c.take<uint64_t>(n);
      d_start_bit = c.take<uint32_t>(n), d_hist = c.take<uint32_t>(n), d_adler_in = c.take<uint32_t>(n);
      d_status = c.take<int32_t>(n);
      d_checksum = c.take<uint32_t>(n), d_resume_adler = c.take<uint32_t>(n), d_resume_last = c.take<uint32_t>(n);
      d_variant = c.take<uint8_t>(n);
    }, 256);
    if (rc != MD_OK) return rc;
    uint8_t *d_out = (uint8_t *)ctx->scratch[kParOut].p;
    if (hl) HIP_TRY(ctx, hipMemcpyAsync(d_out, in.hist, hl, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, md::to_device(d_in_off, in_off.data(), n, st));
    HIP_TRY(ctx, md::to_device(d_in_len, in_len.data(), n, st));
    HIP_TRY(ctx, md::to_device(d_out_off, out_off.data(), n, st));
    HIP_TRY(ctx, md::to_device(d_out_cap, out_cap.data(), n, st));
    HIP_TRY(ctx, md::to_device(d_start_bit, start_bit.data(), n, st));
    HIP_TRY(ctx, md::to_device(d_hist, hist.data(), n, st));
    HIP_TRY(ctx, md::to_device(d_adler_in, adler_in.data(), n, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_variant, variant.data(), n, hipMemcpyHostToDevice, st));
    MD_LAUNCH_TRY(ctx, md_launch_fill_windows((uint32_t)n, d_out, d_out_off, d_variant, st));
    rc = md_inflate_continue_batch_device(ctx, n, d_body, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_start_bit, d_hist, d_adler_in, d_out_len,
                                          d_consumed, d_status, d_checksum, d_resume_bits, d_resume_out, d_resume_adler, d_resume_last);
    if (rc != MD_OK) return rc;
    std::vector<uint64_t> r_used(n), r_bits(n), r_out(n);
    std::vector<int32_t> r_st(n);
    std::vector<uint32_t> r_last(n);
    HIP_TRY(ctx, md::to_host(r_used.data(), d_consumed, n, st));
    HIP_TRY(ctx, md::to_host(r_bits.data(), d_resume_bits, n, st));
    HIP_TRY(ctx, md::to_host(r_out.data(), d_resume_out, n, st));
    HIP_TRY(ctx, md::to_host(r_st.data(), d_status, n, st));
    HIP_TRY(ctx, md::to_host(r_last.data(), d_resume_last, n, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    stamp("pieces decoded");
    // The pieces in order: piece p must end - its last complete block - exactly where piece p + 1 starts ("links").  From
    // piece 0, the true start of the stream, an unbroken chain of links IS the stream's chain of blocks.  A candidate its
    // predecessor does not link to goes (all of them in one round: behind a false candidate the verdicts say little, and a
    // true block start dropped by mistake only costs a split), and everything is decoded again.
    bool again = false, chain = true;
    size_t last = np;  // index of the piece that holds the stream's final block
    std::vector<std::pair<uint64_t, uint64_t>> kill;  // candidates at bits (lo, hi] go
    std::vector<uint64_t> add;                        // block starts found by hopping over stored blocks
    // piece p ended its last complete block at bit e, in front of the next candidate: that candidate is no block start.  If
    // the block at e is STORED, so are all candidates inside it and the stored blocks behind it (compressed data inside the
    // plaintext - a tar of .gz files - is stored, and full of real block headers that are not this stream's): hop over
    // them on the host, a read per block, and the block start behind the run is a candidate the finder could not see.
    auto unlinked = [&](size_t p, uint64_t e) {
      uint64_t hi = p + 1 < np ? pc[p + 1].bit : ~0ull;
      std::vector<uint64_t> mid;
      const uint64_t pos = hop_stored(e, &mid);
      if (pos > e) {
        if (pos > hi) hi = pos;
        for (uint64_t c : mid)
          if (c > pc[p].bit) add.push_back(c);
        if (pos < body_len * 8) add.push_back(pos);
      }
      kill.push_back({pc[p].bit, hi == ~0ull ? pc[p].bit : hi});
    };
    total = 0;
    for (size_t p = 0; p < np; p++) {
      const size_t i = p ? 2 * p - 1 : 0;
      const uint64_t base_bits = (pc[p].bit >> 3) * 8;
      if (p && (r_st[i] != r_st[i + 1] || r_out[i] != r_out[i + 1] || r_bits[i] != r_bits[i + 1])) {
        if (chain) return MD_NOT_HANDLED;  // (the two decodes of a piece of the real chain differ in more than the window's bytes)
        if (p + 1 < np) kill.push_back({pc[p].bit, pc[p + 1].bit});
        again = true;
        continue;
      }
      const bool linked = r_st[i] == MD_UNEXPECTED_END_OF_INPUT && p + 1 < np && base_bits + r_bits[i] == pc[p + 1].bit && r_last[i] == 0;
      if (linked) {
        pc[p].u = r_out[i] - hist[i];
        total += pc[p].u;
      } else if (r_st[i] == MD_UNEXPECTED_END_OF_OUTPUT && p) {  // (piece 0 writes into the caller's room: the serial path's error)
        again = true;
        if (chain) {  // a piece of the real chain needs more room (the candidate behind it stays)
          capmul *= 6;
          if (capmul > 1300) return MD_NOT_HANDLED;
        } else if (p + 1 < np) kill.push_back({pc[p].bit, pc[p + 1].bit});  // (behind a false candidate: garbage that expands)
        chain = false;
      } else if (r_st[i] == MD_OK && chain) {  // the final block ended inside this piece: what follows is not the stream's
        pc[p].u = r_out[i] - hist[i];
        total += pc[p].u;
        used_body = (pc[p].bit >> 3) + r_used[i];
        out->resume_bits = base_bits + r_bits[i];
        out->status = MD_OK;
        last = p;
        break;
      } else if (chain && in.partial_ok && p + 1 == np && r_st[i] == MD_UNEXPECTED_END_OF_INPUT) {
        // the input ends inside the last piece: its complete blocks count, the caller goes on from the last block boundary
        pc[p].u = r_out[i] - hist[i];
        total += pc[p].u;
        out->resume_bits = base_bits + r_bits[i];
        out->status = MD_UNEXPECTED_END_OF_INPUT;
        last = p;
        break;
      } else {
        // on the real chain: a piece that runs over the next candidate makes that candidate false; anything else is an
        // error of the stream itself (or a stream that ends inside its last block): the serial path's
        const bool ran_over = r_st[i] == MD_UNEXPECTED_END_OF_INPUT && p + 1 < np && base_bits + r_bits[i] < pc[p + 1].bit;
        if (chain && !ran_over) return MD_NOT_HANDLED;
        if (ran_over) unlinked(p, base_bits + r_bits[i]);
        else if (p + 1 < np) kill.push_back({pc[p].bit, pc[p + 1].bit});
        again = true;
        chain = false;
      }
    }
    if (again) {
      std::vector<ParPiece> keep;
      for (size_t p = 0; p < np; p++) {
        bool dead = false;
        for (const auto &k : kill) dead = dead || (pc[p].bit > k.first && pc[p].bit <= k.second);
        if (!dead) keep.push_back(pc[p]);
      }
      for (uint64_t x : add) keep.push_back(ParPiece{x});  // (block starts read off the stream itself)
      std::sort(keep.begin(), keep.end(), [](const ParPiece &x, const ParPiece &y) { return x.bit < y.bit; });
      keep.erase(std::unique(keep.begin(), keep.end(), [](const ParPiece &x, const ParPiece &y) { return x.bit == y.bit; }), keep.end());
      pc.swap(keep);
      if (pc.size() < 2) return MD_NOT_HANDLED;
      continue;
    }
    if (last == np) return MD_NOT_HANDLED;
    if (last + 1 < np) pc.resize(last + 1);  // (the scratch of the pieces behind it is simply not looked at)
    break;
  }
  const size_t np = pc.size();
  if (total > dst_cap || np < 2) return MD_NOT_HANDLED;
  // -- windows, then every byte
  {
    std::vector<uint64_t> u(np), pos(np);
    uint64_t acc = 0;
    for (size_t p = 0; p < np; p++) {  // (the window the caller handed in counts as output in front of piece 0)
      u[p] = pc[p].u + (p ? 0 : hl);
      pos[p] = acc;
      acc += u[p];
    }
    // the windows: by pointer jumping over the whole chip (a table of 128 KiB per piece, twice, in groups of 1 023 pieces), or -
    // a handful of pieces - by the one-workgroup chain
    const uint32_t kGroup = 1023;
    const bool jumping = np >= 24;
    const size_t win_bytes = ((np * (size_t)32768 + 255) & ~(size_t)255);
    rc = ctx->scratch[kParWin].reserve(ctx, win_bytes + (jumping ? md_windows_work_bytes((uint32_t)np, kGroup) : 0) + 64,
              "hipMalloc(parallel inflate windows)");
    if (rc != MD_OK) return rc;
    uint64_t *d_offa = nullptr, *d_offb = nullptr, *d_u = nullptr, *d_pos = nullptr;
    uint32_t *d_flag = nullptr;
    rc = carve(ctx, ctx->scratch[kParDesc], "hipMalloc(parallel inflate descriptors)", [&](md::Carver &c) {
      d_offa = c.take<uint64_t>(np), d_offb = c.take<uint64_t>(np), d_u = c.take<uint64_t>(np), d_pos = c.take<uint64_t>(np);
      d_flag = c.take<uint32_t>(16);
    }, 256);
    if (rc != MD_OK) return rc;
    uint8_t *d_out = (uint8_t *)ctx->scratch[kParOut].p, *d_win = (uint8_t *)ctx->scratch[kParWin].p;
    HIP_TRY(ctx, md::to_device(d_offa, offa.data(), np, st));
    HIP_TRY(ctx, md::to_device(d_offb, offb.data(), np, st));
    HIP_TRY(ctx, md::to_device(d_u, u.data(), np, st));
    HIP_TRY(ctx, md::to_device(d_pos, pos.data(), np, st));
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 64, st));
    if (jumping)
      MD_LAUNCH_TRY(ctx, md_launch_windows_parallel((uint32_t)np, kGroup, d_out, u[0], d_out, d_offa, d_offb, d_u, d_pos, d_win, (uint32_t *)(d_win + win_bytes),
                                                    d_flag, st));
    else MD_LAUNCH_TRY(ctx, md_launch_window_chain((uint32_t)np, d_out, d_out, d_offa, d_offb, d_u, d_win, d_flag, st));
    if (dbg_t) {
      hipStreamSynchronize(st);
      stamp("window chain");
    }
    MD_LAUNCH_TRY(ctx, md_launch_resolve((uint32_t)np, d_out, d_out, d_offa, d_offb, d_u, d_pos, d_win, d_flag, st));
    // (the flag is read by the caller together with what it needs next)
    uint32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    stamp("windows + resolve");
    if (flag) return MD_NOT_HANDLED;  // a reference in front of the stream's start
  }
  out->total = total;
  out->used_body = used_body;
  ctx->par_last_pieces = (int)np;
  if (starts) {
    starts->clear();
    uint64_t acc = 0;
    for (size_t p = 1; p < np; p++) {
      acc += pc[p - 1].u;
      starts->push_back(ParStart{pc[p].bit, acc});
    }
  }
  return MD_OK;
}

int continue_parallel_device(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, const uint8_t *hist, size_t hist_len,
                             uint64_t room, const uint8_t **d_out, int *status, uint64_t *total, uint64_t *used, uint64_t *resume_bits,
                             std::vector<ParStart> *starts) {
  ParIn in{src, src_len, start_bit, hist, (uint32_t)hist_len, room, true};
  ParOut po;
  const int rc = par_decode(ctx, in, &po, starts);
  if (rc != MD_OK) return rc;
  *d_out = (const uint8_t *)ctx->scratch[kParOut].p + hist_len;
  *status = po.status;
  *total = po.total;
  *used = po.used_body;
  *resume_bits = po.resume_bits;
  return MD_OK;
}

// Adler-32 of n bytes at d (device) going on from `adler`; CRC-32 of the same bytes (complete value): ctx.hpp
int par_adler(md_ctx *ctx, const uint8_t *d, uint64_t n, uint32_t adler, uint32_t *res) {
  *res = adler;
  if (n == 0) return MD_OK;
  const size_t nseg = (size_t)((n + 65535) / 65536);
  uint32_t *d_sums = nullptr;  // a pair of sums per segment
  const int rc = carve(ctx, ctx->scratch[kParDesc], "hipMalloc(parallel inflate descriptors)", [&](md::Carver &c) {
    d_sums = c.take<uint32_t>(2 * nseg);
  }, 64);
  if (rc != MD_OK) return rc;
  MD_LAUNCH_TRY(ctx, md_launch_adler_segments(d, n, 65536, d_sums, ctx->stream));
  std::vector<uint32_t> sums(2 * nseg);
  HIP_TRY(ctx, md::to_host(sums.data(), d_sums, sums.size(), ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t a = adler & 0xffffu, b = adler >> 16;
  for (size_t s = 0; s < nseg; s++) {
    const uint64_t len = s + 1 < nseg ? 65536 : n - (uint64_t)s * 65536;
    b = (b + (len % 65521) * a + sums[2 * s + 1]) % 65521;
    a = (a + sums[2 * s]) % 65521;
  }
  *res = (uint32_t)((b << 16) | a);
  return MD_OK;
}
int par_crc(md_ctx *ctx, const uint8_t *d_base, uint64_t off, uint64_t n, uint32_t *res) {
  *res = 0;
  if (n == 0) return MD_OK;
  const size_t ncrc = (size_t)((n + ((1u << 20) - 1)) >> 20);
  uint64_t *d_off = nullptr, *d_len = nullptr;
  uint32_t *d_crc = nullptr;
  const int rc = carve(ctx, ctx->scratch[kParDesc], "hipMalloc(parallel inflate descriptors)", [&](md::Carver &c) {
    d_off = c.take<uint64_t>(ncrc), d_len = c.take<uint64_t>(ncrc);
    d_crc = c.take<uint32_t>(ncrc);
  }, 64);
  if (rc != MD_OK) return rc;
  std::vector<uint64_t> co(ncrc), cl(ncrc);
  for (size_t s = 0; s < ncrc; s++) {
    co[s] = off + ((uint64_t)s << 20);
    cl[s] = s + 1 < ncrc ? (uint64_t)1 << 20 : n - ((uint64_t)s << 20);
  }
  HIP_TRY(ctx, md::to_device(d_off, co.data(), ncrc, ctx->stream));
  HIP_TRY(ctx, md::to_device(d_len, cl.data(), ncrc, ctx->stream));
  MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)ncrc, d_base, d_off, d_len, d_crc, ctx->stream));
  std::vector<uint32_t> crcs(ncrc);
  HIP_TRY(ctx, md::to_host(crcs.data(), d_crc, ncrc, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint32_t crc = crcs[0];
  for (size_t s = 1; s < ncrc; s++) crc = md::crc32_concat(crc, crcs[s], cl[s]);
  *res = crc;
  return MD_OK;
}

// md_de_inf_continue_host on a long piece: the blocks that are complete in it by par_decode; if the piece ends inside a
// block, that tail goes through the serial path from the block boundary on (window = the bytes just decoded), so what the
// caller sees - status, the output reached inside the incomplete block, the resume point, the checksums there - is what
// the serial path alone would have said.
int continue_parallel(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, uint8_t *dst, size_t hist_len,
                      size_t dst_cap, uint32_t adler_in, unsigned flags, size_t *dst_len, int *status, md_inf_resume *resume) {
  ParIn in{src, src_len, start_bit, dst, (uint32_t)hist_len, dst_cap - hist_len, true};
  ParOut po;
  int rc = par_decode(ctx, in, &po);
  if (rc != MD_OK) return rc;
  const uint8_t *d_out = (const uint8_t *)ctx->scratch[kParOut].p;
  const int pieces = ctx->par_last_pieces, rounds = ctx->par_last_rounds;
  uint32_t adler = adler_in, crc = 0;
  rc = par_adler(ctx, d_out + hist_len, po.total, adler_in, &adler);
  if (rc == MD_OK && (flags & MD_CONT_CRC32)) rc = par_crc(ctx, d_out, hist_len, po.total, &crc);
  if (rc != MD_OK) return rc;
  if (po.total) HIP_TRY(ctx, hipMemcpy(dst + hist_len, d_out + hist_len, po.total, hipMemcpyDeviceToHost));
  const uint64_t O = hist_len + po.total;  // output position behind the last complete block
  if (po.status == MD_OK) {
    *dst_len = (size_t)O;
    *status = MD_OK;
    resume->bits = po.resume_bits;
    resume->out = O;
    resume->adler = adler;
    resume->last = 1;
    resume->consumed = po.used_body;
    resume->checksum = adler;
    resume->crc_out = resume->crc_end = crc;
    return MD_OK;
  }
  // the tail, serially: from bit B on, with the last 32 KiB in front of it as its window - in place
  const uint64_t B = po.resume_bits, hl2 = O < 32768 ? O : 32768, shift = O - hl2;
  size_t t_len = 0;
  int t_st = 0;
  md_inf_resume t;
  rc = continue_serial(ctx, src + (B >> 3), src_len - (size_t)(B >> 3), (unsigned)(B & 7), dst + shift, (size_t)hl2, dst_cap - (size_t)shift, adler,
                       flags, &t_len, &t_st, &t);
  if (rc != MD_OK) return rc;
  *dst_len = (size_t)shift + t_len;
  *status = t_st;
  resume->bits = (B >> 3) * 8 + t.bits;
  resume->out = shift + t.out;
  resume->adler = t.adler;
  resume->last = t.last;
  resume->consumed = t_st == MD_OK ? (B >> 3) + t.consumed : t.consumed;  // (0 unless the stream ended: no offset then)
  resume->checksum = t.checksum;
  if (flags & MD_CONT_CRC32) {
    const uint64_t n_out = t.out - hl2, n_end = t_len - hl2;
    resume->crc_out = po.total ? (n_out ? md::crc32_concat(crc, t.crc_out, n_out) : crc) : t.crc_out;
    resume->crc_end = po.total ? (n_end ? md::crc32_concat(crc, t.crc_end, n_end) : crc) : t.crc_end;
  } else resume->crc_out = resume->crc_end = 0;
  ctx->par_last_pieces = pieces;
  ctx->par_last_rounds = rounds;
  return MD_OK;
}

int inflate_parallel(md_ctx *ctx, int format, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                     size_t *consumed, size_t *written, uint32_t *checksum) {
  // -- the frame: anything but a plain valid header is the serial path's (it knows the reference's answer)
  size_t hdr = 0, trailer = 0;
  if (format == MD_FORMAT_ZLIB) {
    if (src_len < 6 || (((uint32_t)src[0] << 8) + src[1]) % 31 != 0 || (src[0] & 0xf) != 8) return MD_NOT_HANDLED;
    hdr = 2;
    trailer = 4;
  } else if (format == MD_FORMAT_GZIP) {
    md::gz::InfHeader h;
    if (md::gz::inf_header(src, src_len, &h) != MD_OK || (h.flg & 2)) return MD_NOT_HANDLED;  // (a header CRC: serial path)
    hdr = h.body;
    trailer = 8;
  } else if (format != MD_FORMAT_DEFLATE) return MD_NOT_HANDLED;
  if (src_len < hdr + trailer) return MD_NOT_HANDLED;
  ParIn in{src + hdr, src_len - hdr, 0, nullptr, 0, dst_cap, false};  // (the trailer's bytes included: where the stream ends is the decoder's to say)
  ParOut po;
  int rc = par_decode(ctx, in, &po);
  if (rc != MD_OK) return rc;
  const uint64_t total = po.total, used_body = po.used_body;
  if (src_len - hdr - used_body < trailer) {
    ctx->par_last_pieces = 0;
    return MD_NOT_HANDLED;
  }
  const uint8_t *d_out = (const uint8_t *)ctx->scratch[kParOut].p;
  const uint8_t *t = src + hdr + used_body;
  bool good = true;
  if (format == MD_FORMAT_ZLIB || (format == MD_FORMAT_DEFLATE && checksum)) {
    uint32_t adler = 1;
    rc = par_adler(ctx, d_out, total, 1u, &adler);
    if (rc != MD_OK) return rc;
    if (format == MD_FORMAT_ZLIB) {
      good = md::be32(t) == adler;
    }
    if (checksum) *checksum = adler;
  } else if (format == MD_FORMAT_GZIP) {
    uint32_t crc = 0;
    rc = par_crc(ctx, d_out, 0, total, &crc);
    if (rc != MD_OK) return rc;
    good = md::le32(t) == crc && md::le32(t + 4) == (uint32_t)total;
    if (checksum) *checksum = crc;
  }
  if (!good) {  // the serial path reports it
    ctx->par_last_pieces = 0;
    return MD_NOT_HANDLED;
  }
  if (total) HIP_TRY(ctx, hipMemcpy(dst, d_out, total, hipMemcpyDeviceToHost));
  *consumed = hdr + (size_t)used_body + trailer;
  *written = (size_t)total;
  return MD_OK;
}
