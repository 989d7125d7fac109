// capi_zindex.cpp — the index of one long stream (mdeflate.h: md_inflate_index_*).  The index itself, its checks and its
// serialised form are the host's (zindex.hpp); building it decodes the stream once, in pieces, with the decoders that
// are there (capi_long_stream.cpp's pieces by the whole chip, or one pair of wavefronts per piece); reading through it is
// a plain batch of pieces (zindex_kernels.hip around md_inflate_continue_batch_device).
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "gz_frame.hpp"
#include "zindex.hpp"

namespace {
using md::zix::kWindow;

// compressed input that one piece of the build hands to the whole-chip decoder (its scratch is about 14 times that)
constexpr size_t kParPieceIn = (size_t)32 << 20;
// pieces of a read's round whose numbers are read back together with the plan's four words
constexpr uint64_t kIdsAhead = 4096;
static_assert(md::zix::kWin == md::zix::kWindow, "one window size: internal.hpp's for the kernels, zindex.hpp's for the host");

// The frame's header on the host (Gz.Inf's walk: gz_frame.hpp; Zl.Inf's two bytes): MD_OK and the body's offset
int frame_header(int format, const uint8_t *s, size_t n, uint64_t *body) {
  *body = 0;
  if (format == MD_FORMAT_DEFLATE) return MD_OK;
  if (format == MD_FORMAT_ZLIB) {
    if (n < 2) return MD_UNEXPECTED_END_OF_INPUT;
    if ((((uint32_t)s[0] << 8) + s[1]) % 31 != 0 || (s[0] & 0xf) != 8) return MD_INVALID_HEADER;
    *body = 2;
    return MD_OK;
  }
  md::gz::InfHeader h;
  const int st = md::gz::inf_header(s, n, &h);
  *body = h.body;
  return st;
}

// The stored blocks that are not final from bit `pos` on, read off the stream (header, padding, LEN, NLEN): the bit behind
// the run - `pos` itself when there is none -, cut once it holds `span` bytes; *payload = the bytes it holds
uint64_t stored_run(const uint8_t *src, uint64_t src_len, uint64_t pos, uint64_t span, uint64_t *payload) {
  *payload = 0;
  while (*payload < span) {
    const uint64_t by = pos >> 3;
    if (by >= src_len) break;
    const uint32_t h = ((uint32_t)src[by] | (by + 1 < src_len ? (uint32_t)src[by + 1] << 8 : 0)) >> (pos & 7);
    if ((h & 1) || (h & 6)) break;  // the final block, or not stored
    const uint64_t at = (pos + 3 + 7) >> 3;
    if (at + 4 > src_len) break;
    const uint32_t len = src[at] | ((uint32_t)src[at + 1] << 8), nlen = src[at + 2] | ((uint32_t)src[at + 3] << 8);
    if ((len ^ nlen) != 0xffffu || at + 4 + len > src_len) break;
    pos = (at + 4 + len) * 8;
    *payload += len;
  }
  return pos;
}

// The stream decoded once, in pieces; x receives the points.  Returns the stream's status (or a call-level error).
int build_index(md_ctx *ctx, int format, const uint8_t *src, size_t src_len, uint64_t span, uint8_t *dst, size_t dst_cap, md_inflate_index *x) {
  uint64_t hdr = 0;
  int st = frame_header(format, src, src_len, &hdr);
  if (st != MD_OK) return st;
  x->info.format = format;
  x->info.src_len = src_len;
  x->info.header_len = hdr;
  x->info.span = span;
  md::zix::add_point(x, 8 * hdr, 0, nullptr);
  hipStream_t stream = ctx->stream;
  std::vector<uint8_t> hist, taken;
  std::vector<ParStart> starts;
  std::vector<uint64_t> k_bit, k_out, k_src;
  std::vector<uint32_t> k_len;
  uint64_t cur = 8 * hdr, out_pos = 0, last_kept = 0, body_end = 0, par_skip_until = 0;
  uint32_t adler = 1, crc = 0;
  size_t sticky = 0;
  int chip_pieces = 0, chip_rounds = 0;  // of the pieces that went to the whole chip ("inflate_parallel_last")
  for (bool done = false; !done;) {
    const uint64_t b0 = cur >> 3, avail = src_len - b0;
    const unsigned sb = (unsigned)(cur & 7);
    if (avail == 0) return MD_UNEXPECTED_END_OF_INPUT;
    const size_t hl = hist.size();
    const uint64_t cap_left = dst ? dst_cap - out_pos : UINT64_MAX, room_max = MD_MAX_STREAM - hl;
    const uint8_t *d_base = nullptr;  // the piece on the device: hl bytes of window, then the new output
    uint64_t produced = 0, used = 0, resume_bits = 0;
    uint32_t piece_adler = adler;
    bool final = false, got = false, by_chip = false;
    starts.clear();
    if (ctx->par_min && avail >= ctx->par_min && b0 >= par_skip_until) {
      // a long piece: its complete blocks by the whole chip, and the verified chain of pieces says where blocks start
      const size_t L = (size_t)std::min<uint64_t>(avail, kParPieceIn);
      const uint64_t room = std::min(std::min<uint64_t>(8 * (uint64_t)L + 65536, cap_left), room_max);
      const uint8_t *d_new = nullptr;
      int pst = MD_OK;
      const int rc = continue_parallel_device(ctx, src + b0, L, sb, hist.data(), hl, room, &d_new, &pst, &produced, &used, &resume_bits, &starts);
      if (rc == MD_OK) {
        got = by_chip = true;
        chip_pieces += ctx->par_last_pieces;
        chip_rounds = std::max(chip_rounds, ctx->par_last_rounds);
        d_base = d_new - hl;
        final = pst == MD_OK;
      } else if (rc != MD_NOT_HANDLED) {
        return rc;
      } else {
        par_skip_until = b0 + L;  // (no candidates, too few, a piece without room ..: these bytes go one block run at a time)
      }
    }
    if (!got) {
      // One pair of wavefronts says only where the LAST complete block of a piece ends, so a piece is sized to hold about
      // `span` bytes of output: the input that the stream so far spent on that much (a quarter of it at the start), and
      // half as much again each time a piece held no complete block.  A run of stored blocks is read off the stream itself
      // and is a piece of exactly its length.  A piece that holds the stream's end says nothing about the blocks in front
      // of it: while a point could still be kept there, the piece is cut by bisection - lo bytes hold no complete block,
      // hi bytes hold the end - until a cut leaves complete blocks and not the end, or none does (one block is left).
      const double per_out = out_pos ? (double)(b0 - hdr) / (double)out_pos : 0.25;
      const uint64_t target = (uint64_t)(per_out * (double)span) + 4096;
      uint64_t stored_payload = 0;
      const uint64_t run_end = stored_run(src, src_len, cur, span, &stored_payload);
      uint64_t want = run_end > cur ? (run_end >> 3) - b0 : std::max<uint64_t>(target, sticky), factor = 1, lo = 0, hi = 0;
      bool settle = false;
      for (;;) {
        const size_t L = (size_t)std::min<uint64_t>(std::min<uint64_t>(avail, MD_MAX_INFLATE_IN), want);
        uint64_t room = (std::max<uint64_t>(std::max<uint64_t>(2 * span, 4 * (uint64_t)L), stored_payload) + 65536) * factor;
        const bool at_max = room >= room_max, limited = room >= cap_left;
        room = std::min(std::min(room, room_max), cap_left);
        InfPiece r;
        const int rc = inflate_piece(ctx, src + b0, L, sb, hist.data(), hl, room, adler, &r);
        if (rc != MD_OK) return rc;
        const int pst = r.status;
        d_base = (const uint8_t *)ctx->scratch[kContOut].p;
        if (pst == MD_OK) {
          if (!settle && out_pos + (r.out_len - hl) >= last_kept + span && L - lo > 1) {
            hi = L;
            want = lo + (hi - lo) / 2;
            continue;
          }
          final = true;
          produced = r.out_len - hl;
          used = r.consumed;
          piece_adler = r.checksum;
          break;
        }
        if (r.resume_bits > sb) {  // a complete block: on from its end, whatever stopped the piece behind it
          produced = r.resume_out - hl;
          resume_bits = r.resume_bits;
          piece_adler = r.resume_adler;
          break;
        }
        if (pst == MD_UNEXPECTED_END_OF_INPUT) {
          if (hi) {
            lo = L;
            settle = hi - lo <= 1;
            want = settle ? hi : lo + (hi - lo) / 2;
            continue;
          }
          if (L == avail || L >= MD_MAX_INFLATE_IN) return pst;
          sticky = L + L / 2;
          want = std::max<uint64_t>(target, sticky);
        } else if (pst == MD_UNEXPECTED_END_OF_OUTPUT) {
          if (limited || at_max) return pst;
          factor *= 4;
        } else {
          return pst;
        }
      }
    }
    // the block starts this piece taught, in order: kept when `span` bytes of output lie between
    if (!final) starts.push_back(ParStart{resume_bits, produced});
    k_bit.clear(), k_out.clear(), k_src.clear(), k_len.clear();
    for (const ParStart &s : starts) {
      const uint64_t o = out_pos + s.out;
      if (o < last_kept + span) continue;
      const uint64_t w = md::zix::window_len(o);
      k_bit.push_back(b0 * 8 + s.bit);
      k_out.push_back(o);
      k_src.push_back(hl + s.out - w);  // (hl + s.out bytes lie in front of the point on the device: hl = min(32 KiB, out_pos))
      k_len.push_back((uint32_t)w);
      last_kept = o;
    }
    if (!k_bit.empty()) {
      const size_t m = k_bit.size();
      int rc = ctx->scratch[kZixWin].reserve(ctx, m * kWindow, "hipMalloc(index windows)");
      if (rc != MD_OK) return rc;
      uint64_t *d_src = nullptr;
      uint32_t *d_len = nullptr;
      const auto takes = [&](md::Carver &c) { d_src = c.take<uint64_t>(m), d_len = c.take<uint32_t>(m); };
      rc = carve(ctx, ctx->scratch[kZixDesc], "hipMalloc(index descriptors)", takes, 64);
      if (rc != MD_OK) return rc;
      uint8_t *d_wins = ctx->scratch[kZixWin].as<uint8_t>();
      HIP_TRY(ctx, md::to_device(d_src, k_src, stream));
      HIP_TRY(ctx, md::to_device(d_len, k_len, stream));
      MD_LAUNCH_TRY(ctx, md_launch_zix_windows_take((uint32_t)m, d_base, d_src, d_len, d_wins, stream));
      taken.resize(m * kWindow);
      HIP_TRY(ctx, md::to_host(taken.data(), d_wins, taken.size(), stream));
      HIP_TRY(ctx, hipStreamSynchronize(stream));
      for (size_t p = 0; p < m; p++) md::zix::add_point(x, k_bit[p], k_out[p], taken.data() + p * kWindow);
    }
    // the checksum goes on over the new bytes; the bytes go out if they are wanted
    if (format == MD_FORMAT_GZIP) {
      if (produced) {
        uint32_t c = 0;
        const int rc = par_crc(ctx, d_base, hl, produced, &c);
        if (rc != MD_OK) return rc;
        crc = out_pos ? md::crc32_concat(crc, c, produced) : c;
      }
    } else if (by_chip) {
      const int rc = par_adler(ctx, d_base + hl, produced, adler, &adler);
      if (rc != MD_OK) return rc;
    } else {
      adler = piece_adler;
    }
    if (dst && produced) HIP_TRY(ctx, hipMemcpyAsync(dst + out_pos, d_base + hl, produced, hipMemcpyDeviceToHost, stream));
    if (final) {
      body_end = b0 + used;
      done = true;
    } else {  // the window of the next piece
      const size_t w = (size_t)std::min<uint64_t>(kWindow, hl + produced);
      std::vector<uint8_t> next(w);
      if (w) HIP_TRY(ctx, hipMemcpyAsync(next.data(), d_base + hl + produced - w, w, hipMemcpyDeviceToHost, stream));
      HIP_TRY(ctx, hipStreamSynchronize(stream));
      hist.swap(next);
      cur = b0 * 8 + resume_bits;
    }
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    out_pos += produced;
  }
  // the trailer, as Zl.Inf and Gz.Inf read it (CRC-32 first, then ISIZE)
  const uint64_t trailer = md::zix::trailer_len(format);
  if (src_len - body_end < trailer) return MD_UNEXPECTED_END_OF_INPUT;
  const uint8_t *t = src + body_end;
  if (format == MD_FORMAT_ZLIB && md::be32(t) != adler) return MD_INVALID_CHECKSUM;
  if (format == MD_FORMAT_GZIP) {
    if (md::le32(t) != crc) return MD_INVALID_CHECKSUM;
    if (md::le32(t + 4) != (uint32_t)out_pos) return MD_INVALID_SIZE;
  }
  ctx->par_last_pieces = chip_pieces;
  ctx->par_last_rounds = chip_rounds;
  x->info.consumed = body_end + trailer;
  x->info.size = out_pos;
  x->info.checksum = format == MD_FORMAT_GZIP ? crc : adler;
  return MD_OK;
}
}  // namespace

int md_inflate_index_build(md_ctx *ctx, int format, const uint8_t *src, size_t src_len, uint64_t span, uint8_t *dst, size_t dst_cap,
                           md_inflate_index **idx, md_inflate_index_info *info) {
  if (idx) *idx = nullptr;
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!idx || (!src && src_len)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_inflate_index_build: null pointer");
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP) return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown format");
  if (span == 0) span = md::zix::kSpanDefault;
  if (span < md::zix::kSpanMin || span > MD_MAX_STREAM / 4) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_inflate_index_build: span is 0 or at least 4096");
  if (src_len >> 60) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_inflate_index_build: src_len");
  MD_ON_DEVICE(ctx);
  md_inflate_index *x = new (std::nothrow) md_inflate_index();
  if (!x) return fail(ctx, MD_E_OUT_OF_MEMORY, "md_inflate_index_build");
  const int rc = no_bad_alloc(ctx, "md_inflate_index_build", [&] { return build_index(ctx, format, src, src_len, span, dst, dst ? dst_cap : 0, x); });
  if (rc != MD_OK) {
    delete x;
    return rc;
  }
  if (info) *info = x->info;
  *idx = x;
  return MD_OK;
}

int md_inflate_index_get(const md_inflate_index *idx, md_inflate_index_info *info) {
  if (!idx || !info) return MD_E_INVALID_ARGUMENT;
  *info = idx->info;
  return MD_OK;
}

int md_inflate_index_points(const md_inflate_index *idx, uint64_t *bit, uint64_t *out, size_t cap) {
  if (!idx || (cap && (!bit || !out))) return MD_E_INVALID_ARGUMENT;
  const size_t m = std::min(cap, idx->bit.size());
  for (size_t k = 0; k < m; k++) {
    bit[k] = idx->bit[k];
    out[k] = idx->out[k];
  }
  return MD_OK;
}

size_t md_inflate_index_save_size(const md_inflate_index *idx) { return idx ? md::zix::save_size(idx) : 0; }

int md_inflate_index_save(const md_inflate_index *idx, uint8_t *buf, size_t cap, size_t *len) {
  if (!idx || !len || (!buf && cap)) return MD_E_INVALID_ARGUMENT;
  *len = md::zix::save_size(idx);
  if (*len > cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  md::zix::save(idx, buf);
  return MD_OK;
}

int md_inflate_index_load(const uint8_t *buf, size_t len, md_inflate_index **idx) {
  if (idx) *idx = nullptr;
  if (!idx || (!buf && len)) return MD_E_INVALID_ARGUMENT;
  try {
    return md::zix::load(buf, len, idx);
  } catch (const std::bad_alloc &) {
    return MD_E_OUT_OF_MEMORY;
  }
}

void md_inflate_index_free(md_inflate_index *idx) { delete idx; }

int md_inflate_index_last(const md_ctx *ctx, md_inflate_index_stats *stats) {
  if (!ctx || !stats) return MD_E_INVALID_ARGUMENT;
  *stats = ctx->zix_last;
  return MD_OK;
}

int md_inflate_index_read(md_ctx *ctx, const md_inflate_index *idx, const uint8_t *src, size_t src_len, size_t n, const uint64_t *off,
                          const uint64_t *len, uint8_t *dst, const uint64_t *dst_off, int32_t *status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!idx || (!src && src_len) || (n && (!off || !len || !dst_off || !status))) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_inflate_index_read: null pointer");
  if (n > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many ranges in one call");
  const md_inflate_index_info &f = idx->info;
  if (src_len != f.src_len) return fail(ctx, MD_INVALID_INDEX, "md_inflate_index_read: the index was built from a src of another length");
  // the ranges' bytes are packed back to back on the device, in the order given: what is adjacent in dst leaves by one copy
  std::vector<uint64_t> pack(n);
  uint64_t total = 0, longest = 0;
  for (size_t i = 0; i < n; i++) {
    if (off[i] > f.size || len[i] > f.size - off[i]) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_inflate_index_read: a range ends behind the output");
    pack[i] = total;
    total += len[i];
    longest = std::max(longest, len[i]);
  }
  if (total && !dst) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_inflate_index_read: null pointer");
  ctx->zix_last = {};
  if (n == 0) return MD_OK;
  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  const size_t P = idx->bit.size(), words = (P + 31) / 32;
  // tables, ranges, and the descriptors of a round (at most P pieces), in one block
  md::zix::Tables t{};
  md::zix::Round r{};
  uint64_t *d_off = nullptr, *d_len = nullptr, *d_pack = nullptr, *d_plan = nullptr;
  int32_t *d_status = nullptr;
  uint64_t *d_bit = nullptr, *d_outs = nullptr;
  int rc = carve(ctx, ctx->scratch[kZixDesc], "hipMalloc(index descriptors)", [&](md::Carver &c) {
    d_plan = c.take<uint64_t>(md::zix::kPlanWords);
    d_bit = c.take<uint64_t>(P);
    d_outs = c.take<uint64_t>(P);
    t.place = c.take<uint64_t>(P);
    d_off = c.take<uint64_t>(n);
    d_len = c.take<uint64_t>(n);
    d_pack = c.take<uint64_t>(n);
    uint64_t **r64[8] = {&r.in_off, &r.in_len, &r.out_off, &r.out_cap, &r.out_len, &r.consumed, &r.resume_bits, &r.resume_out};
    for (uint64_t **q : r64) *q = c.take<uint64_t>(P);
    uint32_t **r32[7] = {&r.start_bit, &r.hist_len, &r.adler_in, &r.checksum, &r.resume_adler, &r.resume_last, &r.piece};
    for (uint32_t **q : r32) *q = c.take<uint32_t>(P);
    r.status = c.take<int32_t>(P);
    t.marked = c.take<uint32_t>(words);
    t.round_of = c.take<uint32_t>(P);
    t.verdict = c.take<int32_t>(P);
    d_status = c.take<int32_t>(n);
  }, 64);
  if (rc == MD_OK) rc = ctx->scratch[kZixOut].reserve(ctx, total + 64, "hipMalloc(index ranges)");
  if (rc != MD_OK) return rc;
  t.points = P;
  t.size = f.size;
  t.body_end = f.consumed - md::zix::trailer_len(f.format);
  t.bit = d_bit;
  t.out = d_outs;
  HIP_TRY(ctx, md::to_device(d_bit, idx->bit.data(), P, st));
  HIP_TRY(ctx, md::to_device(d_outs, idx->out.data(), P, st));
  HIP_TRY(ctx, md::to_device(d_off, off, n, st));
  HIP_TRY(ctx, md::to_device(d_len, len, n, st));
  HIP_TRY(ctx, md::to_device(d_pack, pack, st));
  HIP_TRY(ctx, md::zero(t.marked, words, st));
  HIP_TRY(ctx, hipMemsetAsync(t.round_of, 0xff, P * sizeof *t.round_of, st));
  HIP_TRY(ctx, md::zero(d_status, n, st));
  uint8_t *d_dst = ctx->scratch[kZixOut].as<uint8_t>();
  md_inflate_index_stats &stats = ctx->zix_last;
  std::vector<uint32_t> ids;
  uint64_t first = 0;
  for (uint32_t round = 0; first < P; round++) {
    // -- plan: which pieces, where their bytes and slots go; the count, the sizes and the pieces' numbers come back
    MD_LAUNCH_TRY(ctx, md_launch_zix_plan(&t, n, d_off, d_len, round == 0, first, ctx->zix_workspace, round, &r, d_plan, st));
    uint64_t plan[md::zix::kPlanWords];
    // (the pieces' numbers ride along with the four words: up to kIdsAhead of them, so a round costs one wait unless it is larger)
    const size_t ahead = (size_t)std::min<uint64_t>(P - first, kIdsAhead);
    ids.resize(ahead);
    HIP_TRY(ctx, md::to_host(plan, d_plan, md::zix::kPlanWords, st));
    HIP_TRY(ctx, md::to_host(ids.data(), r.piece, ahead, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const size_t count = (size_t)plan[md::zix::kPlanCount];
    first = plan[md::zix::kPlanNext];
    if (count == 0) break;
    if (count > P || first > P) return fail(ctx, MD_E_HIP, "md_inflate_index_read: plan");
    ids.resize(count);
    if (count > ahead) {
      HIP_TRY(ctx, md::to_host(ids.data() + ahead, r.piece + ahead, count - ahead, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    rc = ctx->scratch[kZixIn].reserve(ctx, plan[md::zix::kPlanIn] + 64, "hipMalloc(index input)");
    if (rc == MD_OK) rc = ctx->scratch[kZixSlots].reserve(ctx, plan[md::zix::kPlanScratch] + 64, "hipMalloc(index slots)");
    if (rc == MD_OK) rc = ctx->scratch[kZixWin].reserve(ctx, count * kWindow, "hipMalloc(index windows)");
    if (rc != MD_OK) return rc;
    uint8_t *d_in = ctx->scratch[kZixIn].as<uint8_t>(), *d_slots = ctx->scratch[kZixSlots].as<uint8_t>(), *d_wins = ctx->scratch[kZixWin].as<uint8_t>();
    // -- upload: the compressed bytes of the marked pieces, where the plan put them, and their windows
    uint64_t at = 0;
    for (size_t j = 0; j < count; j++) {
      const size_t k = ids[j];
      if (k >= P || (j && k <= ids[j - 1])) return fail(ctx, MD_E_HIP, "md_inflate_index_read: plan");
      const uint64_t b0 = idx->bit[k] >> 3, b1 = k + 1 < P ? (idx->bit[k + 1] + 7) >> 3 : t.body_end, in_len = b1 - b0;
      if (at + in_len > plan[md::zix::kPlanIn] || b1 > src_len) return fail(ctx, MD_E_HIP, "md_inflate_index_read: plan");
      HIP_TRY(ctx, md::to_device(d_in + at, src + b0, in_len, st));
      at += md::zix::in_stride(in_len);
      stats.bytes_in += in_len;
    }
    for (size_t j = 0; j < count;) {  // (the windows of a run of consecutive pieces lie back to back in the index)
      size_t e = j + 1;
      const auto full = [&](size_t q) { return idx->win_off[ids[q] + 1] - idx->win_off[ids[q]] == kWindow; };
      while (e < count && ids[e] == ids[e - 1] + 1 && full(e - 1)) e++;
      const uint64_t w0 = idx->win_off[ids[j]], w1 = idx->win_off[ids[e - 1] + 1];
      HIP_TRY(ctx, md::to_device(d_wins + j * kWindow, idx->wins.data() + w0, w1 - w0, st));
      stats.bytes_windows += w1 - w0;
      j = e;
    }
    // -- windows in front of the slots, ONE inflate launch, the verdict per piece, the good bytes into the ranges
    MD_LAUNCH_TRY(ctx, md_launch_zix_windows_put((uint32_t)count, d_wins, &r, d_slots, st));
    rc = md_inflate_continue_batch_device(ctx, count, d_in, r.in_off, r.in_len, d_slots, r.out_off, r.out_cap, r.start_bit, r.hist_len, r.adler_in,
                                          r.out_len, r.consumed, r.status, r.checksum, r.resume_bits, r.resume_out, r.resume_adler, r.resume_last);
    if (rc != MD_OK) return rc;
    MD_LAUNCH_TRY(ctx, md_launch_zix_verdict((uint32_t)count, &t, &r, st));
    MD_LAUNCH_TRY(ctx, md_launch_zix_gather(&t, n, longest, d_off, d_len, round, d_slots, d_dst, d_pack, d_status, st));
    stats.pieces += count;
    stats.launches += 1;
    stats.bytes_scratch += plan[md::zix::kPlanScratch];
  }
  // the statuses first: a range that failed is not copied out (its part of the block holds what an earlier call left)
  HIP_TRY(ctx, md::to_host(status, d_status, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  rc = md::adjacent_runs(n, status, len, dst_off, [&](size_t i, uint64_t bytes) -> int {
    HIP_TRY(ctx, md::to_host(dst + dst_off[i], d_dst + pack[i], bytes, st));
    return MD_OK;
  });
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return MD_OK;
}
