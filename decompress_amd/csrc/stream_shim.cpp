// stream_shim.cpp — the reference's resumable decoder / encoder state machines (`Await / `Flush / `End) above the
// batch C ABI: SURVEY.md 8(b) export item (3).
//
// De.Inf.decode (lib/de.ml:1427-1474, signature lib/de.mli:82-144) and Zl.Def.encode / De.Def.encode's drivers
// (lib/zl.ml:509-555, lib/de.mli:300-412) hand a few KiB to the codec per call; a kernel launch per 64 KiB step
// cannot pay for itself, so the shim keeps the reference's calling protocol on the HOST — it collects the chunks
// the caller supplies through src and runs the HIP path on them in large pieces: a stream that ends before a piece
// (md_inf_chunk_bytes, 8 MiB) is full is ONE batch-of-one launch when the caller signals the end of input (src with
// length 0, as in the reference); a longer stream is decoded piece by piece up to the last block
// boundary inside each piece (md_de_inf_continue_host: starting bit, 32 KiB window and checksum state go in, the
// boundary comes back), so that output is handed out through `Flush steps while input is still arriving and only the
// undecoded tail and the window are kept.  There is no CPU codec here: without a gfx950 device the launch fails and
// the stream reports the call-level error.
//
// Divergence (documented): the kernels have De.Inf.Ns's whole-buffer end-of-input rule; the
// streaming rule of lib/de.ml:941-944 (a final end-of-block code shorter than the longest code is accepted at the
// end of the input) gives the same result on every stream a compressor emits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "ctx.hpp"
#include "inflate_batch.hpp"

// The frame around the DEFLATE body of one stream that is decoded in pieces as it arrives, and the steps on it that
// md_inf_* and md_inf_batch_* share: the GZip / ZLIB header, the bookkeeping of a decoded piece, both trailers with
// the reference's messages, the end-of-input failures and the rule for when the next piece is worth decoding.
struct InfFrame {
  int format = 0;
  std::vector<uint8_t> in;    // the input not decoded yet (once decoding in pieces: the undecoded tail)
  bool eoi = false;           // the end of the input was signalled
  bool hdr_done = false, body_done = false, finished = false;
  int status = MD_OK;         // MD_* status of the stream
  std::string message;        // the reference's `Malformed string, with its numbers
  uint32_t checksum = 0;
  size_t need = 0;            // input buffered before the NEXT piece is decoded (grows when a piece holds no block end)
  unsigned in_bit = 0;        // the next block starts this many bits into in[0]
  uint32_t adler = 1;         // checksum state at the last block boundary
  uint32_t crc = 0;           // GZip: CRC-32 of the output handed out so far
  uint64_t total_out = 0;     // ... and its length
};

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
  s->in.clear();
  s->out.clear();
  s->hist.clear();
  s->message.clear();
  s->o_pos = s->served = s->consumed = 0;
  s->eoi = s->ran = s->piecewise = s->hdr_done = s->body_done = s->finished = false;
  s->status = MD_OK;
  s->checksum = 0;
  s->need = s->chunk;
  s->in_bit = 0;
  s->adler = 1;
  s->crc = 0;
  s->total_out = 0;
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

// where the DEFLATE body of a GZip member begins (Gz.Inf's header walk, lib/gz.ml:465-531: FEXTRA's length is read
// big-endian there); 0 when the header is cut short
static size_t gz_body_offset(const std::vector<uint8_t> &in) {
  if (in.size() < 10) return 0;
  const uint32_t flg = in[3];
  size_t p = 10;
  if (flg & 4) {
    if (in.size() - p < 2) return 0;
    const size_t xl = ((size_t)in[p] << 8) | in[p + 1];
    p += 2;
    if (in.size() - p < xl) return 0;
    p += xl;
  }
  for (int which = 0; which < 2; which++) {
    if (!(flg & (which == 0 ? 8u : 16u))) continue;
    for (;;) {
      if (p >= in.size()) return 0;
      if (in[p++] == 0) break;
    }
  }
  if (flg & 2) {
    if (in.size() - p < 2) return 0;
    p += 2;
  }
  return p;
}

// The reference's `Malformed string for a frame whose trailer disagrees: "Invalid checksum (expect:%04lx, has:%04lx)"
// (lib/zl.ml:179-181, lib/gz.ml:287-289: expect = the trailer's value, has = the checksum of what was inflated) and
// "Invalid input size (expect:%ld, inflated:%ld)" (lib/gz.ml:291-293, both as signed 32-bit).  The kernels report the
// status only, so the trailer is looked up here: one more launch of the raw body finds where it ends.
static void inf_detail(md_inf_stream *s) {
  s->message = md_status_string(s->status);
  if (s->status != MD_INVALID_CHECKSUM && s->status != MD_INVALID_SIZE) return;
  const size_t body = s->format == MD_FORMAT_ZLIB ? 2 : gz_body_offset(s->in);
  if (body == 0 || body > s->in.size()) return;
  uint64_t in_off = body, in_len = s->in.size() - body, out_off = 0, out_cap = s->out.size(), out_len = 0, used = 0;
  int32_t st = 0;
  std::vector<uint8_t> scratch(s->out.size() + 16);
  if (md_inflate_batch_host(s->ctx, MD_FORMAT_DEFLATE, 1, s->in.data(), s->in.size(), &in_off, &in_len, scratch.data(),
                            scratch.size(), &out_off, &out_cap, &out_len, &used, &st, nullptr) != MD_OK || st != MD_OK)
    return;
  const size_t t = body + (size_t)used;
  char buf[96];
  if (s->format == MD_FORMAT_ZLIB) {
    if (s->in.size() - t < 4) return;
    const uint32_t expect = ((uint32_t)s->in[t] << 24) | ((uint32_t)s->in[t + 1] << 16) | ((uint32_t)s->in[t + 2] << 8) | s->in[t + 3];
    snprintf(buf, sizeof buf, "Invalid checksum (expect:%04lx, has:%04lx)", (unsigned long)expect, (unsigned long)s->checksum);
  } else {
    if (s->in.size() - t < 8) return;
    const uint32_t crc = (uint32_t)s->in[t] | ((uint32_t)s->in[t + 1] << 8) | ((uint32_t)s->in[t + 2] << 16) | ((uint32_t)s->in[t + 3] << 24);
    const uint32_t isize = (uint32_t)s->in[t + 4] | ((uint32_t)s->in[t + 5] << 8) | ((uint32_t)s->in[t + 6] << 16) | ((uint32_t)s->in[t + 7] << 24);
    if (s->status == MD_INVALID_CHECKSUM)
      snprintf(buf, sizeof buf, "Invalid checksum (expect:%04lx, has:%04lx)", (unsigned long)crc, (unsigned long)s->checksum);
    else
      snprintf(buf, sizeof buf, "Invalid input size (expect:%ld, inflated:%ld)", (long)(int32_t)isize, (long)(int32_t)(uint32_t)out_len);
  }
  s->message = buf;
}

static void inf_run(md_inf_stream *s) {
  // The output size is not known.  A DEFLATE stream expands at most 1032 times: a small input gets room for that at
  // once (one launch whatever its ratio); a GZip member says its size (mod 2^32) in its last four bytes; otherwise
  // start from 4x the input and grow fourfold while the codec runs out of room (5 launches at the worst ratio).
  const uint64_t n_in = s->in.size();
  uint64_t cap = n_in * 4 + 65536;
  if (n_in * 1032 <= (64u << 20)) cap = n_in * 1032 + 65536;
  else if (s->format == MD_FORMAT_GZIP && n_in >= 18) {
    const uint8_t *t = s->in.data() + n_in - 4;
    const uint64_t isize = (uint64_t)t[0] | ((uint64_t)t[1] << 8) | ((uint64_t)t[2] << 16) | ((uint64_t)t[3] << 24);
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

// Gz.Inf's header walk with its checks (lib/gz.ml:463-491, as gz_header_kernel does it for the batch path): the offset
// of the body, or 0 with *st = MD_OK when the header is not all there yet, or 0 with the status of a bad header
static size_t gz_header_check(const std::vector<uint8_t> &in, int *st) {
  *st = MD_OK;
  // (the reference looks at the ID bytes only once the ten fixed bytes are there, lib/gz.ml:463-491: a cut header of
  // fewer bytes is "unexpected end of input" whatever its first bytes are)
  if (in.size() >= 10 && (in[0] != 0x1f || in[1] != 0x8b)) {
    *st = MD_INVALID_GZIP_HEADER;
    return 0;
  }
  const size_t body = gz_body_offset(in);
  if (body == 0) return 0;
  const uint32_t flg = in[3];
  if (flg & 2) {  // FHCRC: the upper half of the CRC-32 of the fixed bytes + name + comment (FEXTRA excluded), big-endian
    uint32_t c = md::crc32_update(0, in.data(), 10);
    size_t p = 10;
    if (flg & 4) p += 2 + (((size_t)in[10] << 8) | in[11]);
    c = md::crc32_update(c, in.data() + p, body - 2 - p);
    const uint32_t want = (c & 0xffff0000u) >> 16, have = ((uint32_t)in[body - 2] << 8) | in[body - 1];
    if (want != have) {
      *st = MD_INVALID_GZIP_HEADER_CHECKSUM;
      return 0;
    }
  }
  return body;
}

// ---- the frame steps (md_inf_* below, md_inf_batch_* further down) ----
static void frame_fail(InfFrame *f, int st) {
  f->status = st;
  f->message = md_status_string(st);
  f->finished = true;
}
// the GZip / ZLIB header, once: true when `in` starts at the DEFLATE body; otherwise the stream waits for more input
// (need) or failed
static bool frame_head(InfFrame *f) {
  const bool final = f->eoi;
  if (f->format == MD_FORMAT_GZIP && !f->hdr_done) {
    int hst = MD_OK;
    const size_t body = gz_header_check(f->in, &hst);
    if (hst != MD_OK) return frame_fail(f, hst), false;
    if (body == 0) {
      if (final) frame_fail(f, MD_UNEXPECTED_END_OF_INPUT);
      else f->need = f->in.size() + 1;
      return false;
    }
    f->in.erase(f->in.begin(), f->in.begin() + body);
    f->hdr_done = true;
  }
  if (f->format == MD_FORMAT_ZLIB && !f->hdr_done) {  // Zl.Inf's header, lib/zl.ml:142-165 (as the kernel checks it)
    if (f->in.size() < 2) {
      if (final) frame_fail(f, MD_UNEXPECTED_END_OF_INPUT);
      else f->need = 2;
      return false;
    }
    const unsigned cmf = f->in[0], flg = f->in[1];
    if (((cmf << 8) + flg) % 31 != 0 || (cmf & 0xf) != 8) return frame_fail(f, MD_INVALID_HEADER), false;
    f->in.erase(f->in.begin(), f->in.begin() + 2);
    f->hdr_done = true;
  }
  return true;
}
// output that a piece hands out: the GZip CRC-32 goes on over it
static void frame_took(InfFrame *f, uint32_t crc_piece, uint64_t len) {
  f->crc = f->total_out ? md::crc32_concat(f->crc, crc_piece, len) : crc_piece;
  f->total_out += len;
}
// the piece ended inside a block before the end of the input: what lies before that block went out, the input from the
// block boundary (bits from in[0], in_bit included) stays.  A new attempt only once input beyond the undecoded tail has
// arrived - that tail holds no complete block, decoding it again alone could not find one - and, when the piece held no
// block end at all, only once the buffered input has doubled (one long block fed in small pieces is decoded again a
// logarithmic number of times, not once per piece).
static void frame_continue(InfFrame *f, uint64_t bits, uint32_t crc_piece, uint64_t len, uint32_t adler, size_t chunk) {
  const bool progress = bits > f->in_bit;
  frame_took(f, crc_piece, len);
  f->adler = adler;
  f->in.erase(f->in.begin(), f->in.begin() + (size_t)(bits >> 3));
  f->in_bit = (unsigned)(bits & 7);
  f->need = progress ? (f->in.size() + 1 > chunk ? f->in.size() + 1 : chunk) : (f->in.size() * 2 > chunk ? f->in.size() * 2 : chunk);
}
// the body ended (status MD_OK; `consumed` bytes of `in`) or failed with `st`; everything decoded went out, also in front
// of an error.  True when a trailer follows.
static bool frame_body_end(InfFrame *f, int st, uint32_t crc_piece, uint64_t len, uint32_t sum, uint64_t consumed) {
  frame_took(f, crc_piece, len);
  f->checksum = f->format == MD_FORMAT_GZIP ? f->crc : sum;
  if (st != MD_OK) return frame_fail(f, st), false;
  f->body_done = true;
  f->in.erase(f->in.begin(), f->in.begin() + (size_t)consumed);
  f->in_bit = 0;
  if (f->format == MD_FORMAT_DEFLATE) {
    f->status = MD_OK;
    f->finished = true;
    return false;
  }
  return true;
}
// the trailer after the body: the stream ends here, or waits for the rest of the trailer (need)
static void frame_trailer(InfFrame *f) {
  const bool final = f->eoi;
  if (f->format == MD_FORMAT_GZIP) {  // Gz.Inf's trailer (lib/gz.ml:344-356): CRC-32 first, then ISIZE, little-endian
    if (f->in.size() < 8) {
      if (final) frame_fail(f, MD_UNEXPECTED_END_OF_INPUT);
      else f->need = 8;
      return;
    }
    const uint8_t *t = f->in.data();
    const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    char msg[96];
    f->status = MD_OK;
    if (crc != f->crc) {
      snprintf(msg, sizeof msg, "Invalid checksum (expect:%04lx, has:%04lx)", (unsigned long)crc, (unsigned long)f->crc);
      f->status = MD_INVALID_CHECKSUM;
      f->message = msg;
    } else if (isize != (uint32_t)f->total_out) {
      snprintf(msg, sizeof msg, "Invalid input size (expect:%ld, inflated:%ld)", (long)(int32_t)isize, (long)(int32_t)(uint32_t)f->total_out);
      f->status = MD_INVALID_SIZE;
      f->message = msg;
    }
    f->in.erase(f->in.begin(), f->in.begin() + 8);
    f->finished = true;
    return;
  }
  // Zl.Inf's trailer: the Adler-32 of the output, big-endian (lib/zl.ml:171-186)
  if (f->in.size() < 4) {
    if (final) frame_fail(f, MD_UNEXPECTED_END_OF_INPUT);
    else f->need = 4;
    return;
  }
  const uint32_t expect = ((uint32_t)f->in[0] << 24) | ((uint32_t)f->in[1] << 16) | ((uint32_t)f->in[2] << 8) | f->in[3];
  f->in.erase(f->in.begin(), f->in.begin() + 4);
  if (expect != f->checksum) {
    char msg[96];
    snprintf(msg, sizeof msg, "Invalid checksum (expect:%04lx, has:%04lx)", (unsigned long)expect, (unsigned long)f->checksum);
    f->status = MD_INVALID_CHECKSUM;
    f->message = msg;
  } else {
    f->status = MD_OK;
  }
  f->finished = true;
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
    uint64_t cap = (uint64_t)hl + s->in.size() * 4 + 65536;
    std::vector<uint8_t> buf;
    size_t dst_len = 0;
    int st = 0;
    md_inf_resume rs;
    static const uint8_t none = 0;
    for (;;) {
      if (cap > MD_MAX_STREAM) cap = MD_MAX_STREAM;
      buf.resize((size_t)cap);
      if (hl) memcpy(buf.data(), s->hist.data(), hl);
      const int rc = md_de_inf_continue_host(s->ctx, s->in.empty() ? &none : s->in.data(), s->in.size(), s->in_bit, buf.data(), hl,
                                             (size_t)cap, s->adler, s->format == MD_FORMAT_GZIP ? MD_CONT_CRC32 : 0u, &dst_len, &st, &rs);
      if (rc != MD_OK) return frame_fail(s, rc);
      if (st == MD_UNEXPECTED_END_OF_OUTPUT && cap < MD_MAX_STREAM) {
        cap *= 4;
        continue;
      }
      break;
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

// ---- the encoder side: Zl.Def.encoder / Gz.Def.encoder / De.Higher's loop with `Manual src and dst ----
}  // extern "C"

namespace {
constexpr size_t kKeepBytes = 65536;             // text behind the end of a piece that the next launch sees again
constexpr size_t kSrcMax = (size_t)1 << 30;      // most that one md_def_src hands over
}  // namespace

struct md_def_stream {
  md_ctx *ctx;
  int format;
  md_deflate_params params;
  md_gz_header gz;
  std::vector<char> name, comment;
  uint8_t *o;
  size_t o_len, o_pos;
  md_piece *dev;               // device side: text of the launch in flight, state, command queue, output of the piece
  std::vector<uint8_t> text;   // the input at absolute positions [w0, w0 + text.size())
  uint64_t w0, launched;       // ...of which [w0, launched) went through a launch already
  uint64_t origin;             // what the device counts positions from (they are 32-bit there): it moves up as the stream grows
  size_t out_len, served;      // output of the last launch (in device memory) / how much of it was handed out
  bool eoi, first, done;
  int status;
  uint32_t checksum;
};

extern "C" {

md_def_stream *md_def_encoder(md_ctx *ctx, int format, const md_deflate_params *params, uint8_t *o, size_t o_len) {
  if (!ctx || !params || !o || o_len == 0) return nullptr;
  // format, level, queue (a power of two >= 4), driver, matcher, window: refused here (md_last_error_string says
  // why), not at the end of the input — Zl.Def.encoder raises Invalid_argument at construction too (lib/de.ml:2286-2288)
  if (md_validate_deflate_params(ctx, format, params) != MD_OK) return nullptr;
  md_piece *dev = md_i_piece_open(ctx, params->queue_len);
  if (!dev) return nullptr;
  md_def_stream *s = new md_def_stream();
  s->ctx = ctx;
  s->format = format;
  s->params = *params;
  if (params->gz_header) {  // keep our own copy of the caller's strings
    s->gz = *params->gz_header;
    if (s->gz.filename) {
      s->name.assign(s->gz.filename, s->gz.filename + strlen(s->gz.filename) + 1);
      s->gz.filename = s->name.data();
    }
    if (s->gz.comment) {
      s->comment.assign(s->gz.comment, s->gz.comment + strlen(s->gz.comment) + 1);
      s->gz.comment = s->comment.data();
    }
    s->params.gz_header = &s->gz;
  }
  s->o = o;
  s->o_len = o_len;
  s->o_pos = s->served = s->out_len = 0;
  s->dev = dev;
  s->w0 = s->launched = s->origin = 0;
  s->eoi = s->done = false;
  s->first = true;
  s->status = MD_OK;
  s->checksum = format == MD_FORMAT_GZIP ? 0u : 1u;
  return s;
}
void md_def_free(md_def_stream *s) {
  if (!s) return;
  md_i_piece_close(s->ctx, s->dev);
  delete s;
}
int md_def_src(md_def_stream *s, const uint8_t *buf, size_t off, size_t len) {
  if (!s || (!buf && len) || s->eoi) return MD_E_INVALID_ARGUMENT;
  if (s->done && s->status != MD_OK) return MD_E_INVALID_ARGUMENT;  // (an encoder that ended with an error takes no more input)
  if (len == 0) {
    s->eoi = true;
    return MD_OK;
  }
  if (len > kSrcMax) return MD_E_INVALID_ARGUMENT;  // (one launch takes what has arrived: positions within it are 32-bit)
  // ... and so is the text that waits for md_def_encode: src calls without an encode in between must not pile up more than
  // one launch can take (mdeflate.h: call md_def_encode between sources; it launches what has arrived)
  if ((s->w0 + s->text.size()) - s->launched + len > kSrcMax) return MD_E_INVALID_ARGUMENT;
  s->text.insert(s->text.end(), buf + off, buf + off + len);
  s->checksum = s->format == MD_FORMAT_GZIP ? md::crc32_update(s->checksum, buf + off, len) : md::adler32_update(s->checksum, buf + off, len);
  return MD_OK;
}
void md_def_dst(md_def_stream *s, uint8_t *o, size_t o_len) {  // Zl.Def.dst: a fresh output buffer
  if (!s || !o || !o_len) return;
  s->o = o;
  s->o_len = o_len;
  s->o_pos = 0;
}
size_t md_def_dst_rem(const md_def_stream *s) { return s ? s->o_len - s->o_pos : 0; }
int md_def_status(const md_def_stream *s) { return s ? s->status : MD_E_INVALID_ARGUMENT; }
uint32_t md_def_checksum(const md_def_stream *s) { return s ? s->checksum : 0; }

// one launch over what has arrived: its output waits in device memory for md_def_encode to hand it out
static void def_launch(md_def_stream *s) {
  const uint64_t end = s->w0 + s->text.size();
  const size_t fresh = (size_t)(end - s->launched), ql = (size_t)s->params.queue_len;
  // room: the commands the queue held back at 6 bytes each (a match: two codes of 15 bits, 5 + 13 extra bits), the fresh
  // bytes at 2 bytes each (a literal is 15 bits at most, a match covers 3 bytes), a block header per queue fill, the frame
  const size_t blocks = (fresh + ql) / ql + 2, per_block = ql >= 128 ? 320 : 24 + 4 * ql;
  const size_t cap = 2048 + 6 * ql + 2 * fresh + blocks * per_block;
  // the device's positions are 32-bit: once the text is 2 GiB from their origin the origin moves up to 64 KiB below it
  // (deflate_test_flags bit 4: at 128 KiB already, so that a test of ordinary size goes through it)
  const uint64_t far = (s->ctx->test_flags & 16) ? (uint64_t)1 << 17 : (uint64_t)1 << 31;
  uint64_t rebase = 0;
  if (s->w0 - s->origin >= far) {
    rebase = (s->w0 - s->origin - 65536) & ~(uint64_t)65535;
    s->origin += rebase;
  }
  int st = 0;
  const int rc = md_i_piece_run(s->ctx, s->dev, s->format, &s->params, s->text.data(), s->text.size(), (size_t)(s->launched - s->w0),
                                s->w0 - s->origin, rebase,
                                s->first, s->eoi, s->checksum, (uint32_t)end, cap, &s->out_len, &st);
  s->first = false;
  s->served = 0;
  s->launched = end;
  if (rc != MD_OK || (st != MD_OK && st != MD_PIECE_AWAIT)) {
    s->status = rc != MD_OK ? rc : st;
    s->out_len = 0;
    s->done = true;
    return;
  }
  if (st == MD_OK) s->done = true;  // (the last piece: trailer written)
  // the next launch sees the last 64 KiB again (the matcher reaches 32 KiB - 262 behind a position it has yet to take,
  // and those are less than 262 from the end): the text before goes
  if (end > kKeepBytes) {
    const uint64_t nw0 = (end - kKeepBytes) & ~(uint64_t)63;
    if (nw0 > s->w0) {
      s->text.erase(s->text.begin(), s->text.begin() + (size_t)(nw0 - s->w0));
      s->w0 = nw0;
    }
  }
}

int md_def_encode(md_def_stream *s) {
  if (!s) return MD_MALFORMED;
  for (;;) {
    if (s->served < s->out_len) {
      const size_t left = s->out_len - s->served, room = s->o_len - s->o_pos;
      const size_t k = left < room ? left : room;
      if (k && md_i_piece_out(s->ctx, s->dev, s->served, s->o + s->o_pos, k) != MD_OK) {
        s->status = MD_E_HIP;
        s->done = true;
        s->out_len = s->served = 0;
        return MD_MALFORMED;
      }
      s->o_pos += k;
      s->served += k;
      if (s->served < s->out_len) return MD_FLUSH;
    }
    if (s->done) return s->status == MD_OK ? MD_END : MD_MALFORMED;
    const size_t fresh = (size_t)(s->w0 + s->text.size() - s->launched);
    // (a launch costs three kernels whatever it holds: input is gathered, 1 MiB unless md_set_option "encoder_piece_bytes")
    if (!s->eoi && fresh < s->ctx->piece_bytes) return MD_AWAIT;
    def_launch(s);
  }
}


// ---- many streaming encoders at once (md_def_batch_*, mdeflate.h) ------------------------------------------------------
// n independent Zl.Def / Gz.Def / De.Def encoders (lib/zl.ml:509-555) with the same parameters whose pieces go through the
// kernels TOGETHER: one launch of the three kernels per md_def_batch_encode whatever n is (md_def_* is one launch per
// encoder and piece), and an encoder's window - the last 64 KiB of its text - STAYS in device memory: only the bytes that
// arrived since the launch before cross the link, packed into one copy.  The text of launch k + 1 is gathered on the device
// from the tail of launch k's and the fresh bytes (piece_gather_kernel); state, queue, rebasing and the `Await protocol
// are the single encoder's (def_launch above, struct Piece), so the bytes of every encoder are those of md_def_* - and of
// the reference - handed the same pieces.
struct md_def_batch {
  md_ctx *ctx = nullptr;
  int format = 0;
  md_deflate_params params{};
  md_gz_header gz{};
  std::vector<char> name, comment;
  size_t n = 0;
  struct Enc {
    std::vector<uint8_t> fresh;   // input handed over since the last launch
    uint64_t w0 = 0, end = 0;     // the device holds the text of absolute positions [w0, end) ...
    uint64_t text_off = 0;        // ... at this offset of the current text blob
    uint64_t origin = 0;          // what the device counts this stream's positions from (32-bit there)
    bool eoi = false, first = true, done = false, launched_eoi = false;
    int status = MD_OK;
    uint32_t checksum = 0;
    uint64_t out_off = 0, out_len = 0, served = 0;  // output of the last launch in the device's output blob
    std::vector<uint8_t> held;    // output of earlier launches that was not fetched before the next one
  };
  std::vector<Enc> e;
  md::DevBuf d_text[2];
  int cur = 0;
  md::DevBuf d_fresh, d_out, d_state, d_queue, d_desc, d_gdesc;
  md::PinnedBuf h_stage;          // the fresh bytes of a launch, packed
};

md_def_batch *md_def_batch_open(md_ctx *ctx, int format, const md_deflate_params *params, size_t n) {
  if (!ctx || !params || n == 0 || n > 0x7fffffffu) return nullptr;
  if (md_validate_deflate_params(ctx, format, params) != MD_OK) return nullptr;
  md::DeviceGuard guard(ctx->device);
  md_def_batch *b = new md_def_batch();
  b->ctx = ctx;
  b->format = format;
  b->params = *params;
  if (params->gz_header) {
    b->gz = *params->gz_header;
    if (b->gz.filename) {
      b->name.assign(b->gz.filename, b->gz.filename + strlen(b->gz.filename) + 1);
      b->gz.filename = b->name.data();
    }
    if (b->gz.comment) {
      b->comment.assign(b->gz.comment, b->gz.comment + strlen(b->gz.comment) + 1);
      b->gz.comment = b->comment.data();
    }
    b->params.gz_header = &b->gz;
  }
  b->n = n;
  b->e.resize(n);
  for (auto &x : b->e) x.checksum = format == MD_FORMAT_GZIP ? 0u : 1u;
  if (b->d_state.reserve(ctx, n * (size_t)md::defl::kPieceState, nullptr) != MD_OK ||
      b->d_queue.reserve(ctx, n * (size_t)params->queue_len * 4, nullptr) != MD_OK) {
    delete b;
    return nullptr;
  }
  return b;
}
void md_def_batch_close(md_def_batch *b) {
  if (!b) return;
  md::DeviceGuard guard(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  delete b;
}
int md_def_batch_src(md_def_batch *b, size_t i, const uint8_t *buf, size_t len) {
  if (!b || i >= b->n || (!buf && len)) return MD_E_INVALID_ARGUMENT;
  md_def_batch::Enc &x = b->e[i];
  if (x.eoi || x.done) return MD_E_INVALID_ARGUMENT;  // (an encoder that ended, also with an error, takes no more input)
  if (len == 0) {
    x.eoi = true;
    return MD_OK;
  }
  if (x.fresh.size() + len > kSrcMax) return MD_E_INVALID_ARGUMENT;  // (what one launch takes: call md_def_batch_encode in between)
  x.fresh.insert(x.fresh.end(), buf, buf + len);
  x.checksum = b->format == MD_FORMAT_GZIP ? md::crc32_update(x.checksum, buf, len) : md::adler32_update(x.checksum, buf, len);
  return MD_OK;
}
size_t md_def_batch_pending(const md_def_batch *b, size_t i) {
  if (!b || i >= b->n) return 0;
  const md_def_batch::Enc &x = b->e[i];
  return x.held.size() + (size_t)(x.out_len - x.served);
}
int md_def_batch_status(const md_def_batch *b, size_t i) {  // the signal md_def_encode would give
  if (!b || i >= b->n) return MD_MALFORMED;
  const md_def_batch::Enc &x = b->e[i];
  if (x.done) return x.status == MD_OK ? MD_END : MD_MALFORMED;
  return MD_AWAIT;
}
int md_def_batch_error(const md_def_batch *b, size_t i) {  // the MD_* status behind MD_MALFORMED (MD_OK otherwise)
  if (!b || i >= b->n) return MD_E_INVALID_ARGUMENT;
  return b->e[i].status;
}
uint32_t md_def_batch_checksum(const md_def_batch *b, size_t i) { return b && i < b->n ? b->e[i].checksum : 0; }
size_t md_def_batch_out(md_def_batch *b, size_t i, uint8_t *dst, size_t cap) {
  if (!b || i >= b->n || (!dst && cap)) return 0;
  md_def_batch::Enc &x = b->e[i];
  size_t got = 0;
  if (!x.held.empty()) {
    const size_t k = x.held.size() < cap ? x.held.size() : cap;
    memcpy(dst, x.held.data(), k);
    x.held.erase(x.held.begin(), x.held.begin() + k);
    got = k;
  }
  if (got < cap && x.served < x.out_len) {
    md::DeviceGuard guard(b->ctx->device);
    const size_t left = (size_t)(x.out_len - x.served), k = left < cap - got ? left : cap - got;
    if (hipMemcpy(dst + got, b->d_out.as<const uint8_t>() + x.out_off + x.served, k, hipMemcpyDeviceToHost) != hipSuccess) return got;
    x.served += k;
    got += k;
  }
  return got;
}
// One launch over what has arrived for every encoder since the last one.  Encoders without new input (and whose end of
// input has not been signalled since) sit the launch out.  MD_OK, or the call-level error.
int md_def_batch_encode(md_def_batch *b) {
  if (!b) return MD_E_INVALID_ARGUMENT;
  md::DeviceGuard guard(b->ctx->device);
  hipStream_t st = b->ctx->stream;
  const size_t n = b->n, ql = (size_t)b->params.queue_len;
  // output that was not fetched yet moves to the host: the launch writes a new output blob
  for (size_t i = 0; i < n; i++) {
    md_def_batch::Enc &x = b->e[i];
    if (x.served < x.out_len) {
      const size_t k = (size_t)(x.out_len - x.served), at = x.held.size();
      x.held.resize(at + k);
      if (hipMemcpy(x.held.data() + at, b->d_out.as<const uint8_t>() + x.out_off + x.served, k, hipMemcpyDeviceToHost) != hipSuccess) return MD_E_HIP;
    }
    x.out_len = x.served = 0;
  }
  std::vector<uint64_t> text_off(n), text_len(n), abs_len(n), out_off(n), out_cap(n), w0(n), rebase(n, 0), out_len(n, 0), g(6 * n);
  std::vector<uint32_t> flags(n), sum(n), isize(n);
  std::vector<int32_t> status(n, 0);
  const uint64_t far = (b->ctx->test_flags & 16) ? (uint64_t)1 << 17 : (uint64_t)1 << 31;
  uint64_t tpos = 0, fpos = 0, opos = 0;
  uint32_t skip = 0xffffffffu;
  size_t active = 0;
  for (size_t i = 0; i < n; i++) {
    md_def_batch::Enc &x = b->e[i];
    const bool act = !x.done && (!x.fresh.empty() || (x.eoi && !x.launched_eoi));
    const uint64_t keep = x.end - x.w0, fresh = act ? x.fresh.size() : 0;
    g[6 * i] = x.text_off;
    g[6 * i + 1] = x.done ? 0 : keep;
    g[6 * i + 2] = fpos;
    g[6 * i + 3] = fresh;
    g[6 * i + 4] = tpos;
    g[6 * i + 5] = 0;
    fpos += (fresh + 15) & ~(uint64_t)15;
    if (act) {
      if (x.w0 - x.origin >= far) {  // 32-bit positions on the device: the origin moves up (def_launch above)
        rebase[i] = (x.w0 - x.origin - 65536) & ~(uint64_t)65535;  // (committed to x.origin only once the launch has succeeded:
      }                                                             //  a call that fails before it leaves every encoder retryable)
      const uint64_t origin = x.origin + rebase[i];
      const uint64_t end = x.end + fresh;
      const size_t blocks = (fresh + ql) / ql + 2, per_block = ql >= 128 ? 320 : 24 + 4 * ql;
      out_cap[i] = 2048 + 6 * ql + 2 * fresh + blocks * per_block;
      flags[i] = (x.first ? 1u : 0u) | (x.eoi ? 2u : 0u);
      abs_len[i] = end - origin;
      w0[i] = x.w0 - origin;
      isize[i] = (uint32_t)end;
      const uint64_t seen = keep;
      const uint32_t sk = seen > 512 ? (uint32_t)(seen - 512) : 0u;
      skip = sk < skip ? sk : skip;
      active++;
    } else {
      flags[i] = 8u;
      out_cap[i] = 16;
      abs_len[i] = w0[i] = 0;
      isize[i] = 0;
    }
    sum[i] = x.checksum;
    text_off[i] = tpos;
    text_len[i] = (x.done ? 0 : keep) + fresh;
    out_off[i] = opos;
    tpos += ((x.done ? 0 : keep) + fresh + 320 + 63) & ~(uint64_t)63;
    opos += (out_cap[i] + 63) & ~(uint64_t)63;
  }
  if (active == 0) return MD_OK;
  const int nxt = b->cur ^ 1;
  int grc = b->d_text[nxt].reserve_blob(b->ctx, (size_t)tpos + 64);
  if (grc == MD_OK) grc = b->d_fresh.reserve_blob(b->ctx, (size_t)fpos + 64);
  if (grc == MD_OK) grc = b->d_out.reserve_blob(b->ctx, (size_t)opos + 64);
  if (grc == MD_OK) grc = b->d_gdesc.reserve_blob(b->ctx, 6 * n * 8);
  if (grc == MD_OK) grc = b->h_stage.reserve(b->ctx, (size_t)fpos + 64, nullptr, md::blob_room((size_t)fpos));
  if (grc != MD_OK) return grc;
  for (size_t i = 0; i < n; i++)
    if (g[6 * i + 3]) memcpy(b->h_stage.as<uint8_t>() + g[6 * i + 2], b->e[i].fresh.data(), (size_t)g[6 * i + 3]);
  if (fpos && hipMemcpyAsync(b->d_fresh.p, b->h_stage.p, (size_t)fpos, hipMemcpyHostToDevice, st) != hipSuccess) return MD_E_HIP;
  if (hipMemcpyAsync(b->d_gdesc.p, g.data(), 6 * n * 8, hipMemcpyHostToDevice, st) != hipSuccess) return MD_E_HIP;
  if (md_launch_piece_gather((uint32_t)n, b->d_text[b->cur].as<const uint8_t>(), b->d_fresh.as<const uint8_t>(), b->d_text[nxt].as<uint8_t>(),
                             b->d_gdesc.as<const uint64_t>(), st) != 0)
    return MD_E_HIP;
  md_pieces_io io{text_off.data(), text_len.data(), abs_len.data(), out_off.data(), out_cap.data(), w0.data(), rebase.data(),
                  flags.data(), sum.data(), isize.data(), out_len.data(), status.data()};
  const int rc = md_i_pieces_run(b->ctx, b->format, &b->params, n, b->d_text[nxt].as<const uint8_t>(), b->d_out.as<uint8_t>(), b->d_state.p,
                                 b->d_queue.p, b->d_desc, &io, skip == 0xffffffffu ? 0u : skip);
  if (rc != MD_OK) return rc;
  b->cur = nxt;
  for (size_t i = 0; i < n; i++) {
    md_def_batch::Enc &x = b->e[i];
    x.text_off = text_off[i];
    if (flags[i] & 8u) continue;
    x.origin += rebase[i];
    x.end += x.fresh.size();
    x.fresh.clear();
    x.first = false;
    if (x.eoi) x.launched_eoi = true;
    if (status[i] != MD_OK && status[i] != MD_PIECE_AWAIT) {
      x.status = status[i];
      x.done = true;
      continue;
    }
    x.out_off = out_off[i];
    x.out_len = out_len[i];
    x.served = 0;
    if (status[i] == MD_OK) x.done = true;  // (the last piece: trailer written)
  }
  // the next launch sees the last 64 KiB of every text again; what lies before goes (the gather takes the tail only)
  for (size_t i = 0; i < n; i++) {
    md_def_batch::Enc &x = b->e[i];
    if (x.done || x.end <= kKeepBytes) continue;
    const uint64_t nw0 = (x.end - kKeepBytes) & ~(uint64_t)63;
    if (nw0 > x.w0) {
      x.text_off += nw0 - x.w0;
      x.w0 = nw0;
    }
  }
  return MD_OK;
}

}  // extern "C"

// ---- many streaming decoders at once (md_inf_batch_*, mdeflate.h) ------------------------------------------------------
// n independent De.Inf / Zl.Inf / Gz.Inf decoders (lib/de.mli:82-144) whose pieces go through the inflate kernel TOGETHER:
// one launch per md_inf_batch_decode over every decoder that has new input, whatever n is.  A decoder's frame - header,
// trailer, the need rule - is md_inf_*'s (the frame_* steps above, on the host, which keeps the undecoded tail as md_inf_*
// keeps `in`); its body is decoded in pieces as md_inf_* decodes it with md_inf_chunk_bytes(1): every piece up to the last
// block boundary inside it.  Between rounds the undecoded tail and the window (the last <= 32 KiB of output) stay in device
// memory, in double-buffered blobs: the input of round k + 1 is gathered from the tails in round k's blob and the bytes that
// arrived since (one packed upload), each output region begins with the window gathered from round k's output blob
// (piece_gather_kernel both times).  The hand-out kernels (inflate_batch.hip) pack what every decoder hands out into one
// blob - with its CRC-32 for GZIP - so that a round costs two copies back: the per-decoder results and the packed output.
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

// One launch of the inflate kernel over `rows` (decoder indices), its hand-out and the two copies back; the results are
// applied to the decoders.  first: the round's launch - every decoder with a body in progress moves to the blobs `nxt`
// (the rows with their fresh bytes); otherwise a launch again for rows whose output room ran out: their input is in place,
// their windows are gathered once more from `old`, behind the *opos bytes of output regions the round has used.
// `grown` gets the rows that ran out of room.
int inf_batch_launch(md_inf_batch *b, const std::vector<size_t> &rows, bool first, int old, int nxt, uint64_t *opos_io,
                     std::vector<size_t> *grown) {
  using md::ib::HandRow;
  hipStream_t st = b->ctx->stream;
  const size_t m = rows.size();
  std::vector<char> is_row(first ? b->n : 0, 0);
  for (size_t i : rows)
    if (first) is_row[i] = 1;
  std::vector<size_t> live;  // the decoders whose tail and window the gathers move
  if (first) {
    for (size_t i = 0; i < b->n; i++) {
      const md_inf_batch::Dec &x = b->d[i];
      if (is_row[i] || (!x.finished && (x.dev_tail || x.win_len))) live.push_back(i);
    }
  } else {
    live = rows;
  }
  const size_t L = live.size();
  // descriptors, u64 words: gather of the inputs (6 L, first only) and of the windows (6 L); per row in_off in_len
  // out_off out_cap, then start_bit hist adler_in flags (u32) - uploaded -; then out_len consumed resume_bits resume_out,
  // status checksum resume_adler resume_last (u32), the HandRows
  const size_t gin_w = first ? 6 * L : 0, up_w = gin_w + 6 * L + 4 * m + 2 * m, all_w = up_w + 4 * m + 2 * m + 6 * m;
  std::vector<uint64_t> desc(up_w, 0);
  uint64_t *gin = desc.data(), *gout = gin + gin_w, *r64 = gout + 6 * L;
  uint32_t *r32 = (uint32_t *)(r64 + 4 * m);
  std::vector<uint64_t> row_of(L, ~(uint64_t)0);  // live index -> row
  {
    std::vector<uint64_t> slot(first ? b->n : 0, 0);
    for (size_t k = 0; k < m; k++)
      if (first) slot[rows[k]] = k;
    for (size_t j = 0; j < L; j++) row_of[j] = first ? (is_row[live[j]] ? slot[live[j]] : ~(uint64_t)0) : j;
  }
  uint64_t ipos = 0, fpos = 0, opos = *opos_io, pack = 0;
  std::vector<uint64_t> moved_in(L), moved_out(L);  // where the decoders that only move go
  for (size_t j = 0; j < L; j++) {
    md_inf_batch::Dec &x = b->d[live[j]];
    const uint64_t k = row_of[j];
    if (first) {
      const uint64_t fresh = k != ~(uint64_t)0 ? x.in.size() - x.dev_tail : 0, len = x.dev_tail + fresh;
      uint64_t *g = gin + 6 * j;
      g[0] = x.tail_off;
      g[1] = x.dev_tail;
      g[2] = fpos;
      g[3] = fresh;
      g[4] = ipos;
      if (k != ~(uint64_t)0) {
        r64[0 * m + k] = ipos;
        r64[1 * m + k] = len;
      } else {
        moved_in[j] = ipos;
      }
      fpos += up(fresh, 16);
      ipos += up(len, 64) + 64;
    }
    uint64_t room = x.win_len;
    if (k != ~(uint64_t)0) {  // md_inf_*'s room for the piece: the window, 4x the input and 64 KiB
      const uint64_t in_len = first ? r64[1 * m + k] : x.in.size();
      uint64_t cap = ((uint64_t)x.win_len + in_len * 4 + 65536) * x.room;
      if (cap > MD_MAX_STREAM || x.room > ((uint64_t)1 << 40)) cap = MD_MAX_STREAM;
      room = cap;
      r64[2 * m + k] = opos;
      r64[3 * m + k] = cap;
      r32[0 * m + k] = x.in_bit;
      r32[1 * m + k] = x.win_len;
      r32[2 * m + k] = x.adler;
      r32[3 * m + k] = (x.eoi ? md::ib::kRowFinal : 0u) | (cap < MD_MAX_STREAM ? md::ib::kRowCanGrow : 0u);
      pack += up(cap - x.win_len, 16);
    }
    uint64_t *g = gout + 6 * j;
    g[0] = x.win_off;
    g[1] = x.win_len;
    g[2] = 0;
    g[3] = 0;
    g[4] = opos;
    moved_out[j] = opos;
    opos += up(room, 64) + 64;
  }
  if (!first) {  // (a retry: the rows' input regions of the round's launch)
    for (size_t k = 0; k < m; k++) {
      r64[0 * m + k] = b->d[rows[k]].tail_off;
      r64[1 * m + k] = b->d[rows[k]].in.size();
    }
  }
  // (a launch again keeps the output regions the round has used)
  int grc = first ? b->d_in[nxt].reserve_blob(b->ctx, (size_t)ipos + 64) : MD_OK;
  if (grc == MD_OK)
    grc = first ? b->d_out[nxt].reserve_blob(b->ctx, (size_t)opos + 64) : b->d_out[nxt].reserve_keep(b->ctx, (size_t)opos + 64, (size_t)*opos_io);
  if (grc == MD_OK) grc = b->d_fresh.reserve_blob(b->ctx, (size_t)fpos + 64);
  if (grc == MD_OK) grc = b->d_desc.reserve_blob(b->ctx, all_w * 8 + 64);
  if (grc == MD_OK) grc = b->d_pack.reserve_blob(b->ctx, (size_t)pack + 64);
  if (grc == MD_OK) grc = b->h_stage.reserve_blob(b->ctx, (size_t)fpos + 64);
  if (grc != MD_OK) return grc;
  if (first) {
    for (size_t j = 0; j < L; j++) {
      const md_inf_batch::Dec &x = b->d[live[j]];
      const uint64_t *g = gin + 6 * j;
      if (g[3]) memcpy(b->h_stage.as<uint8_t>() + g[2], x.in.data() + x.dev_tail, (size_t)g[3]);
    }
    if (fpos && hipMemcpyAsync(b->d_fresh.p, b->h_stage.p, (size_t)fpos, hipMemcpyHostToDevice, st) != hipSuccess) return MD_E_HIP;
  }
  uint64_t *dd = b->d_desc.as<uint64_t>();
  if (hipMemcpyAsync(dd, desc.data(), up_w * 8, hipMemcpyHostToDevice, st) != hipSuccess) return MD_E_HIP;
  if (first && md_launch_piece_gather((uint32_t)L, b->d_in[old].as<const uint8_t>(), b->d_fresh.as<const uint8_t>(), b->d_in[nxt].as<uint8_t>(),
                                      dd, st) != 0)
    return MD_E_HIP;
  if (md_launch_piece_gather((uint32_t)L, b->d_out[old].as<const uint8_t>(), b->d_fresh.as<const uint8_t>(), b->d_out[nxt].as<uint8_t>(),
                             dd + gin_w, st) != 0)
    return MD_E_HIP;
  uint64_t *d64 = dd + gin_w + 6 * L;
  uint32_t *d32 = (uint32_t *)(d64 + 4 * m);
  uint64_t *o64 = d64 + 6 * m;
  uint32_t *o32 = (uint32_t *)(o64 + 4 * m);
  HandRow *dres = (HandRow *)(o64 + 6 * m);
  const int rc = md_inflate_continue_batch_device(b->ctx, m, b->d_in[nxt].as<const uint8_t>(), d64, d64 + m, b->d_out[nxt].as<uint8_t>(),
                                                  d64 + 2 * m, d64 + 3 * m, d32, d32 + m, d32 + 2 * m, o64, o64 + m, (int32_t *)o32,
                                                  o32 + m, o64 + 2 * m, o64 + 3 * m, o32 + 2 * m, o32 + 3 * m);
  if (rc != MD_OK) return rc;
  b->launches++;
  const md::ib::HandIn hin{d64 + 2 * m, d64 + 3 * m, o64, o64 + m, o64 + 2 * m, o64 + 3 * m, d32 + m, d32 + 3 * m, o32 + m, o32 + 2 * m,
                           (const int32_t *)o32};
  if (md_launch_inf_handout((uint32_t)m, hin, b->d_out[nxt].as<const uint8_t>(), dres, b->d_pack.as<uint8_t>(),
                            b->format == MD_FORMAT_GZIP, st) != 0)
    return MD_E_HIP;
  std::vector<HandRow> res(m);
  if (hipMemcpyAsync(res.data(), dres, m * sizeof(HandRow), hipMemcpyDeviceToHost, st) != hipSuccess ||
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
    if (row_of[j] != ~(uint64_t)0) continue;
    b->d[live[j]].tail_off = moved_in[j];
    b->d[live[j]].win_off = moved_out[j];
  }
  for (size_t k = 0; k < m; k++) {
    md_inf_batch::Dec &x = b->d[rows[k]];
    const HandRow &h = res[k];
    const uint64_t in_off = r64[0 * m + k], in_len = r64[1 * m + k], out_off = r64[2 * m + k];
    if (h.kind == md::ib::kKindGrow) {
      x.room *= 4;
      x.tail_off = in_off;  // (the input stays where this launch read it, the window where it was)
      x.dev_tail = (size_t)in_len;
      grown->push_back(rows[k]);
      continue;
    }
    if (h.len) x.held.insert(x.held.end(), b->h_pack.as<uint8_t>() + h.pack_off, b->h_pack.as<uint8_t>() + h.pack_off + h.len);
    if (h.kind == md::ib::kKindContinue) {
      const uint64_t skip = h.tail_bits >> 3, keep = h.end < 32768 ? h.end : 32768;
      frame_continue(&x, h.tail_bits, h.crc, h.len, h.sum, 1);
      x.tail_off = in_off + skip;
      x.dev_tail = (size_t)(in_len - skip);
      x.win_off = out_off + h.end - keep;
      x.win_len = (uint32_t)keep;
      continue;
    }
    x.dev_tail = 0;
    x.win_len = 0;
    if (frame_body_end(&x, h.status, h.crc, h.len, h.sum, h.tail_bits >> 3)) frame_trailer(&x);
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
  if (x.round_in + len > kSrcMax) return MD_E_INVALID_ARGUMENT;  // (what one round takes: call md_inf_batch_decode in between)
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
