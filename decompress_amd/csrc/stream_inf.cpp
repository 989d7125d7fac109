// stream_inf.cpp — the reference's resumable decoder state machine (`Await / `Flush / `End) above the batch C ABI, for
// one stream (md_inf_*) and for many at once (md_inf_batch_*): SURVEY.md 8(b) export item (3).
//
// De.Inf.decode (lib/de.ml:1427-1474, signature lib/de.mli:82-144) hands a few KiB to the codec per call; a kernel
// launch per 64 KiB step cannot pay for itself, so the shim keeps the reference's calling protocol on the HOST — it
// collects the chunks the caller supplies through src and runs the HIP path on them in large pieces: a stream that ends
// before a piece (md_inf_chunk_bytes, 8 MiB) is full is ONE batch-of-one launch when the caller signals the end of input
// (src with length 0, as in the reference); a longer stream is decoded piece by piece up to the last block boundary
// inside each piece (md_de_inf_continue_host: starting bit, 32 KiB window and checksum state go in, the boundary comes
// back), so that output is handed out through `Flush steps while input is still arriving and only the undecoded tail and
// the window are kept.  There is no CPU codec here: without a gfx950 device the launch fails and the stream reports the
// call-level error.  (The encoder's side of the protocol: stream_def.cpp.)
//
// Divergence (documented): the kernels have De.Inf.Ns's whole-buffer end-of-input rule; the
// streaming rule of lib/de.ml:941-944 (a final end-of-block code shorter than the longest code is accepted at the
// end of the input) gives the same result on every stream a compressor emits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ctx.hpp"
#include "inflate_batch.hpp"
#include "stream_frame.hpp"

struct md_inf_stream : InfFrame {
  md_ctx *ctx;
  uint8_t *o;
  size_t o_len, o_pos;        // caller's output buffer (De.Inf.decoder ~o) and how much of it is filled
  std::vector<uint8_t> out;   // the decoded stream, once the launch has run
  size_t served;              // bytes of `out` already handed to the caller
  bool ran;
  size_t consumed;
  // decoding in pieces (DEFLATE / ZLIB / GZIP): `in` is then the undecoded tail, `out` what the last piece produced
  size_t chunk;               // input buffered before a piece is decoded
  bool piecewise;
  std::vector<uint8_t> hist;  // the window: the last <= 32 KiB of output
};
static void inf_clear(md_inf_stream *s) {
  const int format = s->format;
  static_cast<InfFrame &>(*s) = InfFrame();
  s->format = format;
  s->need = s->chunk;
  s->out.clear();
  s->hist.clear();
  s->o_pos = s->served = s->consumed = 0;
  s->ran = s->piecewise = false;
}

extern "C" {

md_inf_stream *md_inf_decoder(md_ctx *ctx, int format, uint8_t *o, size_t o_len) {
  if (!ctx || !o || o_len == 0) return nullptr;
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP) return nullptr;
  md_inf_stream *s = new md_inf_stream();
  s->ctx = ctx;
  s->format = format;
  s->o = o;
  s->o_len = o_len;
  s->chunk = (size_t)8 << 20;  // (pieces this long are decoded by the whole chip: capi_long_stream.cpp continue_parallel)
  inf_clear(s);
  return s;
}

void md_inf_free(md_inf_stream *s) { delete s; }

// De.Inf.reset (lib/de.ml:1512-1532; Zl.Inf.reset, Gz.Inf.reset): the same decoder, output buffer and format, a new stream
void md_inf_reset(md_inf_stream *s) {
  if (s) inf_clear(s);
}
void md_inf_chunk_bytes(md_inf_stream *s, size_t bytes) {
  if (!s || s->piecewise) return;
  s->chunk = s->need = bytes ? bytes : 1;
}

int md_inf_src(md_inf_stream *s, const uint8_t *buf, size_t off, size_t len) {
  if (!s || (!buf && len) || s->eoi) return MD_E_INVALID_ARGUMENT;
  if (len == 0) s->eoi = true;  // De.Inf.src d buf 0 0: the end of the input
  else s->in.insert(s->in.end(), buf + off, buf + off + len);
  return MD_OK;
}

void md_inf_flush(md_inf_stream *s) {
  if (s) s->o_pos = 0;
}
size_t md_inf_dst_rem(const md_inf_stream *s) { return s ? s->o_len - s->o_pos : 0; }
size_t md_inf_src_rem(const md_inf_stream *s) { return s && (s->ran || s->finished) ? s->in.size() - s->consumed : 0; }
int md_inf_status(const md_inf_stream *s) { return s ? s->status : MD_E_INVALID_ARGUMENT; }
const char *md_inf_message(const md_inf_stream *s) {
  if (!s) return "Invalid argument";
  return s->message.empty() ? md_status_string(s->status) : s->message.c_str();
}
uint32_t md_inf_checksum(const md_inf_stream *s) { return s ? s->checksum : 0; }

// The reference's `Malformed string for a stream, decoded in one launch, whose trailer disagrees (frame_bad_checksum,
// frame_bad_size).  The kernels report the status only, so the trailer is looked up here: one more launch of the raw
// body finds where it ends.
static void inf_detail(md_inf_stream *s) {
  s->message = md_status_string(s->status);
  if (s->status != MD_INVALID_CHECKSUM && s->status != MD_INVALID_SIZE) return;
  md::gz::InfHeader gz{};
  if (s->format != MD_FORMAT_ZLIB && md::gz::inf_header(s->in.data(), s->in.size(), &gz) != MD_OK) return;
  const size_t body = s->format == MD_FORMAT_ZLIB ? 2 : gz.body;
  if (body > s->in.size()) return;
  uint64_t in_off = body, in_len = s->in.size() - body, out_off = 0, out_cap = s->out.size(), out_len = 0, used = 0;
  int32_t st = 0;
  std::vector<uint8_t> scratch(s->out.size() + 16);
  if (md_inflate_batch_host(s->ctx, MD_FORMAT_DEFLATE, 1, s->in.data(), s->in.size(), &in_off, &in_len, scratch.data(),
                            scratch.size(), &out_off, &out_cap, &out_len, &used, &st, nullptr) != MD_OK || st != MD_OK)
    return;
  const size_t t = body + (size_t)used;
  if (s->in.size() - t < (s->format == MD_FORMAT_ZLIB ? 4u : 8u)) return;
  const uint8_t *trailer = s->in.data() + t;
  if (s->format == MD_FORMAT_ZLIB) frame_bad_checksum(s, md::be32(trailer), s->checksum);
  else if (s->status == MD_INVALID_CHECKSUM) frame_bad_checksum(s, md::le32(trailer), s->checksum);
  else frame_bad_size(s, md::le32(trailer + 4), (uint32_t)out_len);
}

static void inf_run(md_inf_stream *s) {
  // The output size is not known.  A DEFLATE stream expands at most 1032 times: a small input gets room for that at
  // once (one launch whatever its ratio); a GZip member says its size (mod 2^32) in its last four bytes; otherwise
  // start from 4x the input and grow fourfold while the codec runs out of room (5 launches at the worst ratio).
  const uint64_t n_in = s->in.size();
  uint64_t cap = n_in * 4 + 65536;
  if (n_in * 1032 <= (64u << 20)) cap = n_in * 1032 + 65536;
  else if (s->format == MD_FORMAT_GZIP && n_in >= 18) {
    const uint64_t isize = md::le32(s->in.data() + n_in - 4);
    if (isize >= cap && isize <= n_in * 1032) cap = isize + 65536;
  }
  for (;;) {
    if (cap > MD_MAX_STREAM) cap = MD_MAX_STREAM;
    s->out.resize((size_t)cap);
    uint64_t in_off = 0, in_len = s->in.size(), out_off = 0, out_cap = cap, out_len = 0, used = 0;
    int32_t st = 0;
    uint32_t sum = 0;
    static const uint8_t none = 0;
    int rc = md_inflate_batch_host(s->ctx, s->format, 1, s->in.empty() ? &none : s->in.data(), s->in.size(), &in_off, &in_len,
                                   s->out.data(), (size_t)cap, &out_off, &out_cap, &out_len, &used, &st, &sum);
    if (rc != MD_OK) {
      s->status = rc;
      s->out.clear();
      return;
    }
    if (st == MD_UNEXPECTED_END_OF_OUTPUT && cap < MD_MAX_STREAM) {
      cap *= 4;
      continue;
    }
    s->status = st;
    s->consumed = (size_t)used;
    s->checksum = sum;
    s->out.resize((size_t)out_len);
    if (st != MD_OK) inf_detail(s);
    return;
  }
}

// One piece of a stream that is decoded as it arrives: everything up to the last block boundary inside the buffered
// input goes to `out`, the rest of the input stays; at the end of the input whatever is left is decoded for good.
static void inf_piece(md_inf_stream *s) {
  const bool final = s->eoi;
  s->out.clear();
  s->served = 0;
  if (!frame_head(s)) return;
  if (!s->body_done) {
    const size_t hl = s->hist.size();
    std::vector<uint8_t> buf;
    size_t dst_len = 0;
    int st = 0;
    md_inf_resume rs;
    static const uint8_t none = 0;
    for (uint64_t factor = 1;; factor *= 4) {  // (more room while the piece runs out of it)
      const uint64_t cap = piece_room(hl, s->in.size(), factor);
      buf.resize((size_t)cap);
      if (hl) memcpy(buf.data(), s->hist.data(), hl);
      const int rc = md_de_inf_continue_host(s->ctx, s->in.empty() ? &none : s->in.data(), s->in.size(), s->in_bit, buf.data(), hl,
                                             (size_t)cap, s->adler, s->format == MD_FORMAT_GZIP ? MD_CONT_CRC32 : 0u, &dst_len, &st, &rs);
      if (rc != MD_OK) return frame_fail(s, rc);
      if (st != MD_UNEXPECTED_END_OF_OUTPUT || cap >= MD_MAX_STREAM) break;
    }
    if (st == MD_UNEXPECTED_END_OF_INPUT && !final) {
      // the piece ends inside a block: hand out what lies before that block, keep the rest of the input
      const size_t upto = (size_t)rs.out;
      s->out.assign(buf.begin() + hl, buf.begin() + upto);
      const size_t keep = upto < 32768 ? upto : 32768;
      s->hist.assign(buf.begin() + (upto - keep), buf.begin() + upto);
      frame_continue(s, rs.bits, rs.crc_out, upto - hl, rs.adler, s->chunk);
      return;
    }
    s->out.assign(buf.begin() + hl, buf.begin() + dst_len);  // everything decoded, also in front of an error
    if (!frame_body_end(s, st, rs.crc_end, dst_len - hl, rs.checksum, rs.consumed)) return;
  }
  frame_trailer(s);
}

int md_inf_decode(md_inf_stream *s) {
  if (!s) return MD_MALFORMED;
  for (;;) {
    // what has been decoded goes to the caller's buffer first
    const size_t left = s->out.size() - s->served, room = s->o_len - s->o_pos;
    const size_t n = left < room ? left : room;
    if (n) memcpy(s->o + s->o_pos, s->out.data() + s->served, n);
    s->o_pos += n;
    s->served += n;
    if (s->served < s->out.size() || (n && s->o_pos == s->o_len && s->finished && s->status != MD_OK)) return MD_FLUSH;  // the buffer is full
    if (s->finished) return s->status == MD_OK ? MD_END : MD_MALFORMED;
    if (!s->piecewise && s->eoi) {  // the whole stream in one launch
      inf_run(s);
      s->ran = s->finished = true;
      continue;
    }
    if (!s->eoi && s->in.size() < s->need) return MD_AWAIT;
    s->piecewise = true;
    inf_piece(s);
  }
}

}  // extern "C"

// ---- many streaming decoders at once (md_inf_batch_*, mdeflate.h) ------------------------------------------------------
// n independent De.Inf / Zl.Inf / Gz.Inf decoders (lib/de.mli:82-144) whose pieces go through the inflate kernel TOGETHER:
// one launch per md_inf_batch_decode over every decoder that has new input, whatever n is.  A decoder's frame - header,
// trailer, the need rule - is md_inf_*'s (the frame_* steps of stream_frame.hpp, on the host, which keeps the undecoded tail
// as md_inf_* keeps `in`); its body is decoded in pieces as md_inf_* decodes it with md_inf_chunk_bytes(1): every piece up
// to the last block boundary inside it.  Between rounds the undecoded tail and the window (the last <= 32 KiB of output)
// stay in device memory, in double-buffered blobs: the input of round k + 1 is gathered from the tails in round k's blob
// and the bytes that arrived since (one packed upload), each output region begins with the window gathered from round k's
// output blob (piece_gather_kernel both times).  The hand-out kernels (inflate_batch.hip) pack what every decoder hands out
// into one blob - with its CRC-32 for GZIP - so that a round costs two copies back: the per-decoder results and the packed
// output.
struct md_inf_batch {
  md_ctx *ctx = nullptr;
  int format = 0;
  size_t n = 0;
  struct Dec : InfFrame {
    std::vector<uint8_t> held;  // output handed out and not fetched yet, from held_pos on
    size_t held_pos = 0;
    size_t round_in = 0;        // input handed over since the last md_inf_batch_decode
    // the body in progress on the device: in[0, dev_tail) at tail_off of the current input blob; the window: win_len bytes
    // at win_off of the current output blob
    size_t dev_tail = 0;
    uint64_t tail_off = 0, win_off = 0;
    uint32_t win_len = 0;
    uint64_t room = 1;          // a piece's output room is this multiple of md_inf_*'s (x4 each time it ran out)
    uint64_t attempts = 0;      // rounds the decoder took part in (md_i_inf_batch_attempts)
  };
  std::vector<Dec> d;
  md::DevBuf d_in[2], d_out[2];
  int cur = 0;
  md::DevBuf d_fresh, d_desc, d_pack;
  md::PinnedBuf h_stage, h_pack;  // the fresh bytes of a round, packed / the packed output
  uint64_t launches = 0;      // inflate launches so far (md_i_inf_batch_launches)
};
namespace {
void inf_slot_clear(md_inf_batch::Dec *x, int format) {
  *x = md_inf_batch::Dec();
  x->format = format;
  x->need = 1;  // (md_inf_*'s rule with md_inf_chunk_bytes(1): a piece as soon as input has arrived)
}
uint64_t up(uint64_t x, uint64_t a) { return (x + a - 1) & ~(a - 1); }

// The descriptor blob of one inflate launch over m rows, L decoders of which move: where each array lies, from `base`
// on.  Made twice a launch, over the host's copy and over d_desc, so that both sides' addresses come from this one list.
// The part up to `upload` bytes is what the host fills and sends; the kernels write the rest.
struct InfRound {
  md::GatherRow *gather_in, *gather_out;            // [L] each (gather_in: the round's first launch only)
  uint64_t *in_off, *in_len, *out_off, *out_cap;    // [m] each, as all that follow
  uint32_t *start_bit, *hist, *adler_in, *flags;
  size_t upload;
  uint64_t *out_len, *consumed, *resume_bits, *resume_out;
  int32_t *status;
  uint32_t *checksum, *resume_adler, *resume_last;
  md::ib::HandRow *hand;
  size_t bytes;
  InfRound(void *base, size_t L, size_t m, bool first) {
    md::Carver c(base);
    gather_in = c.take<md::GatherRow>(first ? L : 0), gather_out = c.take<md::GatherRow>(L);
    in_off = c.take<uint64_t>(m), in_len = c.take<uint64_t>(m), out_off = c.take<uint64_t>(m), out_cap = c.take<uint64_t>(m);
    start_bit = c.take<uint32_t>(m), hist = c.take<uint32_t>(m), adler_in = c.take<uint32_t>(m), flags = c.take<uint32_t>(m);
    upload = c.at;
    out_len = c.take<uint64_t>(m), consumed = c.take<uint64_t>(m), resume_bits = c.take<uint64_t>(m), resume_out = c.take<uint64_t>(m);
    status = c.take<int32_t>(m), checksum = c.take<uint32_t>(m), resume_adler = c.take<uint32_t>(m), resume_last = c.take<uint32_t>(m);
    hand = c.take<md::ib::HandRow>(m);
    bytes = c.at;
  }
};

// One launch of the inflate kernel over `rows` (decoder indices), its hand-out and the two copies back; the results are
// applied to the decoders.  first: the round's launch - every decoder with a body in progress moves to the blobs `nxt`
// (the rows with their fresh bytes); otherwise a launch again for rows whose output room ran out: their input is in place,
// their windows are gathered once more from `old`, behind the *opos bytes of output regions the round has used.
// `grown` gets the rows that ran out of room.
int inf_batch_launch(md_inf_batch *b, const std::vector<size_t> &rows, bool first, int old, int nxt, uint64_t *opos_io,
                     std::vector<size_t> *grown) {
  using md::ib::HandRow;
  constexpr uint64_t kNoRow = ~(uint64_t)0;
  hipStream_t st = b->ctx->stream;
  const size_t m = rows.size();
  std::vector<uint64_t> slot(first ? b->n : 0, kNoRow);  // decoder -> row, for the round's launch
  for (size_t k = 0; first && k < m; k++) slot[rows[k]] = k;
  std::vector<size_t> live;  // the decoders whose tail and window the gathers move
  if (first) {
    for (size_t i = 0; i < b->n; i++) {
      const md_inf_batch::Dec &x = b->d[i];
      if (slot[i] != kNoRow || (!x.finished && (x.dev_tail || x.win_len))) live.push_back(i);
    }
  } else {
    live = rows;
  }
  const size_t L = live.size();
  std::vector<uint64_t> desc(InfRound(nullptr, L, m, first).upload / 8, 0);
  const InfRound h(desc.data(), L, m, first);
  std::vector<uint64_t> row_of(L);  // live index -> row
  for (size_t j = 0; j < L; j++) row_of[j] = first ? slot[live[j]] : j;
  uint64_t ipos = 0, fpos = 0, opos = *opos_io, pack = 0;
  std::vector<uint64_t> moved_in(L), moved_out(L);  // where the decoders that only move go
  for (size_t j = 0; j < L; j++) {
    md_inf_batch::Dec &x = b->d[live[j]];
    const uint64_t k = row_of[j];
    if (first) {
      const uint64_t fresh = k != kNoRow ? x.in.size() - x.dev_tail : 0, len = x.dev_tail + fresh;
      h.gather_in[j] = {x.tail_off, x.dev_tail, fpos, fresh, ipos, 0};
      if (k != kNoRow) {
        h.in_off[k] = ipos;
        h.in_len[k] = len;
      } else {
        moved_in[j] = ipos;
      }
      fpos += up(fresh, 16);
      ipos += up(len, 64) + 64;
    }
    uint64_t room = x.win_len;
    if (k != kNoRow) {  // md_inf_*'s room for the piece
      room = piece_room(x.win_len, first ? h.in_len[k] : x.in.size(), x.room);
      h.out_off[k] = opos;
      h.out_cap[k] = room;
      h.start_bit[k] = x.in_bit;
      h.hist[k] = x.win_len;
      h.adler_in[k] = x.adler;
      h.flags[k] = (x.eoi ? md::ib::kRowFinal : 0u) | (room < MD_MAX_STREAM ? md::ib::kRowCanGrow : 0u);
      pack += up(room - x.win_len, 16);
    }
    h.gather_out[j] = {x.win_off, x.win_len, 0, 0, opos, 0};
    moved_out[j] = opos;
    opos += up(room, 64) + 64;
  }
  if (!first) {  // (a retry: the rows' input regions of the round's launch)
    for (size_t k = 0; k < m; k++) {
      h.in_off[k] = b->d[rows[k]].tail_off;
      h.in_len[k] = b->d[rows[k]].in.size();
    }
  }
  // (a launch again keeps the output regions the round has used)
  int grc = first ? b->d_in[nxt].reserve_blob(b->ctx, (size_t)ipos + 64) : MD_OK;
  if (grc == MD_OK)
    grc = first ? b->d_out[nxt].reserve_blob(b->ctx, (size_t)opos + 64) : b->d_out[nxt].reserve_keep(b->ctx, (size_t)opos + 64, (size_t)*opos_io);
  if (grc == MD_OK) grc = b->d_fresh.reserve_blob(b->ctx, (size_t)fpos + 64);
  if (grc == MD_OK) grc = b->d_desc.reserve_blob(b->ctx, h.bytes + 64);
  if (grc == MD_OK) grc = b->d_pack.reserve_blob(b->ctx, (size_t)pack + 64);
  if (grc == MD_OK) grc = b->h_stage.reserve_blob(b->ctx, (size_t)fpos + 64);
  if (grc != MD_OK) return grc;
  if (first) {
    for (size_t j = 0; j < L; j++) {
      const md::GatherRow &g = h.gather_in[j];
      if (g.fresh_len) memcpy(b->h_stage.as<uint8_t>() + g.fresh_off, b->d[live[j]].in.data() + b->d[live[j]].dev_tail, (size_t)g.fresh_len);
    }
    if (fpos && hipMemcpyAsync(b->d_fresh.p, b->h_stage.p, (size_t)fpos, hipMemcpyHostToDevice, st) != hipSuccess) return MD_E_HIP;
  }
  const InfRound d(b->d_desc.p, L, m, first);
  if (hipMemcpyAsync(b->d_desc.p, desc.data(), h.upload, hipMemcpyHostToDevice, st) != hipSuccess) return MD_E_HIP;
  if (first && md_launch_piece_gather((uint32_t)L, b->d_in[old].as<const uint8_t>(), b->d_fresh.as<const uint8_t>(), b->d_in[nxt].as<uint8_t>(),
                                      d.gather_in, st) != 0)
    return MD_E_HIP;
  if (md_launch_piece_gather((uint32_t)L, b->d_out[old].as<const uint8_t>(), b->d_fresh.as<const uint8_t>(), b->d_out[nxt].as<uint8_t>(),
                             d.gather_out, st) != 0)
    return MD_E_HIP;
  const int rc = md_inflate_continue_batch_device(b->ctx, m, b->d_in[nxt].as<const uint8_t>(), d.in_off, d.in_len, b->d_out[nxt].as<uint8_t>(),
                                                  d.out_off, d.out_cap, d.start_bit, d.hist, d.adler_in, d.out_len, d.consumed, d.status,
                                                  d.checksum, d.resume_bits, d.resume_out, d.resume_adler, d.resume_last);
  if (rc != MD_OK) return rc;
  b->launches++;
  const md::ib::HandIn hin{d.out_off, d.out_cap, d.out_len, d.consumed, d.resume_bits, d.resume_out, d.hist, d.flags, d.checksum,
                           d.resume_adler, d.status};
  if (md_launch_inf_handout((uint32_t)m, hin, b->d_out[nxt].as<const uint8_t>(), d.hand, b->d_pack.as<uint8_t>(),
                            b->format == MD_FORMAT_GZIP, st) != 0)
    return MD_E_HIP;
  std::vector<HandRow> res(m);
  if (hipMemcpyAsync(res.data(), d.hand, m * sizeof(HandRow), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return MD_E_HIP;
  const uint64_t total = m ? res[m - 1].pack_off + res[m - 1].len : 0;
  if (total > pack) return MD_E_HIP;  // (cannot happen: every range lies inside its row's room)
  if (total) {
    if (b->h_pack.reserve_blob(b->ctx, (size_t)total) != MD_OK) return MD_E_OUT_OF_MEMORY;
    if (hipMemcpyAsync(b->h_pack.p, b->d_pack.p, (size_t)total, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return MD_E_HIP;
  }
  // the launch went through: the decoders that only moved are at their new places, the rows take their results
  *opos_io = opos;
  for (size_t j = 0; j < L; j++) {
    if (row_of[j] != kNoRow) continue;
    b->d[live[j]].tail_off = moved_in[j];
    b->d[live[j]].win_off = moved_out[j];
  }
  for (size_t k = 0; k < m; k++) {
    md_inf_batch::Dec &x = b->d[rows[k]];
    const HandRow &r = res[k];
    const uint64_t in_off = h.in_off[k], in_len = h.in_len[k], out_off = h.out_off[k];
    if (r.kind == md::ib::kKindGrow) {
      x.room *= 4;
      x.tail_off = in_off;  // (the input stays where this launch read it, the window where it was)
      x.dev_tail = (size_t)in_len;
      grown->push_back(rows[k]);
      continue;
    }
    if (r.len) x.held.insert(x.held.end(), b->h_pack.as<uint8_t>() + r.pack_off, b->h_pack.as<uint8_t>() + r.pack_off + r.len);
    if (r.kind == md::ib::kKindContinue) {
      const uint64_t skip = r.tail_bits >> 3, keep = r.end < 32768 ? r.end : 32768;
      frame_continue(&x, r.tail_bits, r.crc, r.len, r.sum, 1);
      x.tail_off = in_off + skip;
      x.dev_tail = (size_t)(in_len - skip);
      x.win_off = out_off + r.end - keep;
      x.win_len = (uint32_t)keep;
      continue;
    }
    x.dev_tail = 0;
    x.win_len = 0;
    if (frame_body_end(&x, r.status, r.crc, r.len, r.sum, r.tail_bits >> 3)) frame_trailer(&x);
  }
  return MD_OK;
}
}  // namespace

extern "C" {

md_inf_batch *md_inf_batch_open(md_ctx *ctx, int format, size_t n) {
  if (!ctx || n == 0 || n > 0x7fffffffu) return nullptr;
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP) return nullptr;
  md_inf_batch *b = new md_inf_batch();
  b->ctx = ctx;
  b->format = format;
  b->n = n;
  b->d.resize(n);
  for (auto &x : b->d) inf_slot_clear(&x, format);
  return b;
}
void md_inf_batch_close(md_inf_batch *b) {
  if (!b) return;
  md::DeviceGuard guard(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  delete b;
}
int md_inf_batch_src(md_inf_batch *b, size_t i, const uint8_t *buf, size_t len) {
  if (!b || i >= b->n || (!buf && len)) return MD_E_INVALID_ARGUMENT;
  md_inf_batch::Dec &x = b->d[i];
  if (x.eoi || x.finished) return MD_E_INVALID_ARGUMENT;  // (after the end of the input, or of the stream)
  if (len == 0) {
    x.eoi = true;
    return MD_OK;
  }
  if (x.round_in + len > md::kSrcMax) return MD_E_INVALID_ARGUMENT;  // (what one round takes: call md_inf_batch_decode in between)
  x.in.insert(x.in.end(), buf, buf + len);
  x.round_in += len;
  return MD_OK;
}
// One round: the decoders that have input (or its end) beyond what their last attempt saw - md_inf_*'s need rule - take
// their next step, the ones whose body goes on in one launch of the inflate kernel; those whose output room ran out go
// through one more launch with 4x the room, in this call.  Everything else sits the round out; no work, no launch.
int md_inf_batch_decode(md_inf_batch *b) {
  if (!b) return MD_E_INVALID_ARGUMENT;
  std::vector<size_t> rows;
  for (size_t i = 0; i < b->n; i++) {
    md_inf_batch::Dec &x = b->d[i];
    if (x.finished || (!x.eoi && x.in.size() < x.need)) continue;
    x.attempts++;
    if (!frame_head(&x)) continue;
    if (x.body_done) {
      frame_trailer(&x);
      continue;
    }
    if (x.in.size() > MD_MAX_INFLATE_IN) {  // (md_de_inf_continue_host's refusal: bit positions are 32-bit)
      frame_fail(&x, MD_E_INVALID_ARGUMENT);
      x.dev_tail = 0;
      x.win_len = 0;
      continue;
    }
    rows.push_back(i);
  }
  for (auto &x : b->d) x.round_in = 0;
  if (rows.empty()) return MD_OK;
  md::DeviceGuard guard(b->ctx->device);
  const int old = b->cur, nxt = old ^ 1;
  uint64_t opos = 0;
  std::vector<size_t> grown;
  int rc = inf_batch_launch(b, rows, true, old, nxt, &opos, &grown);
  if (rc != MD_OK) return rc;  // (nothing was committed: the decoders try again in the next call)
  b->cur = nxt;
  while (!grown.empty()) {
    std::vector<size_t> again;
    again.swap(grown);
    rc = inf_batch_launch(b, again, false, old, nxt, &opos, &grown);
    if (rc != MD_OK) {  // (the round's other decoders have gone on: these cannot go back)
      for (size_t i : again) {
        frame_fail(&b->d[i], rc);
        b->d[i].dev_tail = 0;
        b->d[i].win_len = 0;
      }
      return rc;
    }
  }
  return MD_OK;
}
size_t md_inf_batch_pending(const md_inf_batch *b, size_t i) {
  if (!b || i >= b->n) return 0;
  return b->d[i].held.size() - b->d[i].held_pos;
}
size_t md_inf_batch_out(md_inf_batch *b, size_t i, uint8_t *dst, size_t cap) {
  if (!b || i >= b->n || (!dst && cap)) return 0;
  md_inf_batch::Dec &x = b->d[i];
  const size_t left = x.held.size() - x.held_pos, k = left < cap ? left : cap;
  if (k) memcpy(dst, x.held.data() + x.held_pos, k);
  x.held_pos += k;
  if (x.held_pos == x.held.size()) {
    x.held.clear();
    x.held_pos = 0;
  } else if (x.held_pos > (1u << 20) && x.held_pos * 2 > x.held.size()) {
    x.held.erase(x.held.begin(), x.held.begin() + x.held_pos);
    x.held_pos = 0;
  }
  return k;
}
int md_inf_batch_status(const md_inf_batch *b, size_t i) {  // the signal md_inf_decode would give once the output is fetched
  if (!b || i >= b->n) return MD_MALFORMED;
  const md_inf_batch::Dec &x = b->d[i];
  if (x.finished) return x.status == MD_OK ? MD_END : MD_MALFORMED;
  return MD_AWAIT;
}
int md_inf_batch_error(const md_inf_batch *b, size_t i) { return b && i < b->n ? b->d[i].status : MD_E_INVALID_ARGUMENT; }
const char *md_inf_batch_message(const md_inf_batch *b, size_t i) {
  if (!b || i >= b->n) return "Invalid argument";
  const md_inf_batch::Dec &x = b->d[i];
  return x.message.empty() ? md_status_string(x.status) : x.message.c_str();
}
uint32_t md_inf_batch_checksum(const md_inf_batch *b, size_t i) { return b && i < b->n ? b->d[i].checksum : 0; }
size_t md_inf_batch_src_rem(const md_inf_batch *b, size_t i) { return b && i < b->n && b->d[i].finished ? b->d[i].in.size() : 0; }
void md_inf_batch_reset(md_inf_batch *b, size_t i) {
  if (b && i < b->n) inf_slot_clear(&b->d[i], b->format);
}
// test hooks (not in mdeflate.h): inflate launches so far; rounds decoder i took part in
long long md_i_inf_batch_launches(const md_inf_batch *b) { return b ? (long long)b->launches : -1; }
long long md_i_inf_batch_attempts(const md_inf_batch *b, size_t i) { return b && i < b->n ? (long long)b->d[i].attempts : -1; }

}  // extern "C"
