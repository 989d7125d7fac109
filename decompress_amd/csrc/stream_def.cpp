
// stream_def.cpp — the reference's resumable encoder state machine (`Await / `Flush / `End) above the batch C ABI, for
// one stream (md_def_*) and for many at once (md_def_batch_*): Zl.Def.encoder / Gz.Def.encoder / De.Higher's loop with
// `Manual src and dst (lib/zl.ml:509-555, lib/de.mli:300-412).  As on the decoder's side (stream_inf.cpp) the calling
// protocol is kept on the HOST: the text the caller supplies through src is gathered and goes through the kernels in
// large pieces, the device carrying the matcher's state from one piece to the next.  The rules of a piece - its output
// room, when the device's origin moves, what text the next piece sees again, the checksum - are stated once, below, for
// both encoders: their bytes are the same, handed the same pieces.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ctx.hpp"

namespace {
constexpr size_t kKeepBytes = 65536;  // text behind the end of a piece that the next launch sees again

// the encoder's own copy of the caller's GZip header and its strings; `params` points at it from then on
struct OwnedGzHeader {
  md_gz_header gz{};
  std::vector<char> name, comment;
  void adopt(md_deflate_params *params) {
    if (!params->gz_header) return;
    gz = *params->gz_header;
    if (gz.filename) {
      name.assign(gz.filename, gz.filename + strlen(gz.filename) + 1);
      gz.filename = name.data();
    }
    if (gz.comment) {
      comment.assign(gz.comment, gz.comment + strlen(gz.comment) + 1);
      gz.comment = comment.data();
    }
    params->gz_header = &gz;
  }
};
// output room of a piece: the commands the queue held back at 6 bytes each (a match: two codes of 15 bits, 5 + 13 extra
// bits), the fresh bytes at 2 bytes each (a literal is 15 bits at most, a match covers 3 bytes), a block header per queue
// fill, the frame
size_t piece_out_cap(size_t fresh, size_t ql) {
  const size_t blocks = (fresh + ql) / ql + 2, per_block = ql >= 128 ? 320 : 24 + 4 * ql;
  return 2048 + 6 * ql + 2 * fresh + blocks * per_block;
}
// the device's positions are 32-bit: once the text (from w0) is 2 GiB from their origin the origin moves up to 64 KiB
// below it, by the amount returned (0: not due).  deflate_test_flags bit 4: at 128 KiB already, so that a test of
// ordinary size goes through it
uint64_t rebase_step(uint64_t w0, uint64_t origin, int test_flags) {
  const uint64_t far = (test_flags & 16) ? (uint64_t)1 << 17 : (uint64_t)1 << 31;
  return w0 - origin >= far ? (w0 - origin - 65536) & ~(uint64_t)65535 : 0;
}
// the next launch sees the last 64 KiB before `end` again (the matcher reaches 32 KiB - 262 behind a position it has yet
// to take, and those are less than 262 from the end): where the text it keeps starts, 64-aligned
uint64_t next_window_start(uint64_t end) { return end > kKeepBytes ? (end - kKeepBytes) & ~(uint64_t)63 : 0; }
// the checksum of the input, by format: CRC-32 for GZip, else Adler-32
uint32_t sum_seed(int format) { return format == MD_FORMAT_GZIP ? 0u : 1u; }
uint32_t sum_update(int format, uint32_t sum, const uint8_t *p, size_t n) {
  return format == MD_FORMAT_GZIP ? md::crc32_update(sum, p, n) : md::adler32_update(sum, p, n);
}
// a piece's status: MD_PIECE_AWAIT (the encoder goes on) and MD_OK (the last piece: trailer written) are the good ones
bool piece_failed(int st) { return st != MD_OK && st != MD_PIECE_AWAIT; }
}  // namespace

struct md_def_stream {
  md_ctx *ctx = nullptr;
  int format = 0;
  md_deflate_params params{};
  OwnedGzHeader own;
  uint8_t *o = nullptr;
  size_t o_len = 0, o_pos = 0;
  md_piece *dev = nullptr;          // device side: text of the launch in flight, state, command queue, output of the piece
  std::vector<uint8_t> text;        // the input at absolute positions [w0, w0 + text.size())
  uint64_t w0 = 0, launched = 0;    // ...of which [w0, launched) went through a launch already
  uint64_t origin = 0;              // what the device counts positions from (they are 32-bit there): it moves up as the stream grows
  size_t out_len = 0, served = 0;   // output of the last launch (in device memory) / how much of it was handed out
  bool eoi = false, first = true, done = false;
  int status = MD_OK;
  uint32_t checksum = 0;
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
  s->own.adopt(&s->params);
  s->o = o;
  s->o_len = o_len;
  s->dev = dev;
  s->checksum = sum_seed(format);
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
  if (len > md::kSrcMax) return MD_E_INVALID_ARGUMENT;  // (one launch takes what has arrived: positions within it are 32-bit)
  // ... and so is the text that waits for md_def_encode: src calls without an encode in between must not pile up more than
  // one launch can take (mdeflate.h: call md_def_encode between sources; it launches what has arrived)
  if ((s->w0 + s->text.size()) - s->launched + len > md::kSrcMax) return MD_E_INVALID_ARGUMENT;
  s->text.insert(s->text.end(), buf + off, buf + off + len);
  s->checksum = sum_update(s->format, s->checksum, buf + off, len);
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
  const size_t cap = piece_out_cap((size_t)(end - s->launched), (size_t)s->params.queue_len);
  const uint64_t rebase = rebase_step(s->w0, s->origin, s->ctx->test_flags);
  s->origin += rebase;
  int st = 0;
  const int rc = md_i_piece_run(s->ctx, s->dev, s->format, &s->params, s->text.data(), s->text.size(), (size_t)(s->launched - s->w0),
                                s->w0 - s->origin, rebase,
                                s->first, s->eoi, s->checksum, (uint32_t)end, cap, &s->out_len, &st);
  s->first = false;
  s->served = 0;
  s->launched = end;
  if (rc != MD_OK || piece_failed(st)) {
    s->status = rc != MD_OK ? rc : st;
    s->out_len = 0;
    s->done = true;
    return;
  }
  if (st == MD_OK) s->done = true;  // (the last piece: trailer written)
  const uint64_t nw0 = next_window_start(end);  // the text before goes
  if (nw0 > s->w0) {
    s->text.erase(s->text.begin(), s->text.begin() + (size_t)(nw0 - s->w0));
    s->w0 = nw0;
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
// are the single encoder's (the piece rules above, struct Piece), so the bytes of every encoder are those of md_def_* -
// and of the reference - handed the same pieces.
struct md_def_batch {
  md_ctx *ctx = nullptr;
  int format = 0;
  md_deflate_params params{};
  OwnedGzHeader own;
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
  b->own.adopt(&b->params);
  b->n = n;
  b->e.resize(n);
  for (auto &x : b->e) x.checksum = sum_seed(format);
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
  if (x.fresh.size() + len > md::kSrcMax) return MD_E_INVALID_ARGUMENT;  // (what one launch takes: call md_def_batch_encode in between)
  x.fresh.insert(x.fresh.end(), buf, buf + len);
  x.checksum = sum_update(b->format, x.checksum, buf, len);
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
  std::vector<uint64_t> text_off(n), text_len(n), abs_len(n), out_off(n), out_cap(n), w0(n), rebase(n, 0), out_len(n, 0);
  std::vector<md::GatherRow> g(n);
  std::vector<uint32_t> flags(n), sum(n), isize(n);
  std::vector<int32_t> status(n, 0);
  uint64_t tpos = 0, fpos = 0, opos = 0;
  uint32_t skip = 0xffffffffu;
  size_t active = 0;
  for (size_t i = 0; i < n; i++) {
    md_def_batch::Enc &x = b->e[i];
    const bool act = !x.done && (!x.fresh.empty() || (x.eoi && !x.launched_eoi));
    const uint64_t keep = x.end - x.w0, fresh = act ? x.fresh.size() : 0;
    g[i] = {x.text_off, x.done ? 0 : keep, fpos, fresh, tpos, 0};
    fpos += (fresh + 15) & ~(uint64_t)15;
    if (act) {
      // (committed to x.origin only once the launch has succeeded: a call that fails before it leaves every encoder retryable)
      rebase[i] = rebase_step(x.w0, x.origin, b->ctx->test_flags);
      const uint64_t origin = x.origin + rebase[i];
      const uint64_t end = x.end + fresh;
      out_cap[i] = piece_out_cap((size_t)fresh, ql);
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
  if (grc == MD_OK) grc = b->d_gdesc.reserve_blob(b->ctx, n * sizeof(md::GatherRow));
  if (grc == MD_OK) grc = b->h_stage.reserve(b->ctx, (size_t)fpos + 64, nullptr, md::blob_room((size_t)fpos));
  if (grc != MD_OK) return grc;
  for (size_t i = 0; i < n; i++)
    if (g[i].fresh_len) memcpy(b->h_stage.as<uint8_t>() + g[i].fresh_off, b->e[i].fresh.data(), (size_t)g[i].fresh_len);
  if (fpos && hipMemcpyAsync(b->d_fresh.p, b->h_stage.p, (size_t)fpos, hipMemcpyHostToDevice, st) != hipSuccess) return MD_E_HIP;
  if (hipMemcpyAsync(b->d_gdesc.p, g.data(), n * sizeof(md::GatherRow), hipMemcpyHostToDevice, st) != hipSuccess) return MD_E_HIP;
  if (md_launch_piece_gather((uint32_t)n, b->d_text[b->cur].as<const uint8_t>(), b->d_fresh.as<const uint8_t>(), b->d_text[nxt].as<uint8_t>(),
                             b->d_gdesc.as<const md::GatherRow>(), st) != 0)
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
    if (piece_failed(status[i])) {
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
    const uint64_t nw0 = x.done ? 0 : next_window_start(x.end);
    if (nw0 > x.w0) {
      x.text_off += nw0 - x.w0;
      x.w0 = nw0;
    }
  }
  return MD_OK;
}

}  // extern "C"
