// stream_frame.hpp — the frame around the DEFLATE body of one stream that is decoded in pieces as it arrives, and the
// steps on it that md_inf_* and md_inf_batch_* (stream_inf.cpp) share: the GZip / ZLIB header, the bookkeeping of a
// decoded piece, both trailers with the reference's messages, the end-of-input failures, the rule for when the next
// piece is worth decoding and the output room a piece gets.  All of it runs on the host.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "ctx.hpp"
#include "gz_frame.hpp"

#pragma GCC visibility push(hidden)

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

// A piece's output room: the window, 4x the input and 64 KiB, times `factor` (x4 each time the piece ran out of it),
// MD_MAX_STREAM at the most
inline uint64_t piece_room(uint64_t window, uint64_t in_len, uint64_t factor) {
  const uint64_t cap = (window + in_len * 4 + 65536) * factor;
  return cap > MD_MAX_STREAM || factor > ((uint64_t)1 << 40) ? MD_MAX_STREAM : cap;
}

// ---- the frame steps ----
inline void frame_fail(InfFrame *f, int st) {
  f->status = st;
  f->message = md_status_string(st);
  f->finished = true;
}
// The reference's `Malformed strings for a frame whose trailer disagrees (lib/zl.ml:179-181, lib/gz.ml:287-289: expect =
// the trailer's value, has = the checksum of what was inflated; lib/gz.ml:291-293: both sizes as signed 32-bit)
inline void frame_bad_checksum(InfFrame *f, uint32_t expect, uint32_t has) {
  char msg[96];
  snprintf(msg, sizeof msg, "Invalid checksum (expect:%04lx, has:%04lx)", (unsigned long)expect, (unsigned long)has);
  f->status = MD_INVALID_CHECKSUM;
  f->message = msg;
}
inline void frame_bad_size(InfFrame *f, uint32_t expect, uint32_t inflated) {
  char msg[96];
  snprintf(msg, sizeof msg, "Invalid input size (expect:%ld, inflated:%ld)", (long)(int32_t)expect, (long)(int32_t)inflated);
  f->status = MD_INVALID_SIZE;
  f->message = msg;
}
// the GZip / ZLIB header, once: true when `in` starts at the DEFLATE body; otherwise the stream waits for more input
// (need) or failed
inline bool frame_head(InfFrame *f) {
  const bool final = f->eoi;
  if (f->format == MD_FORMAT_GZIP && !f->hdr_done) {
    md::gz::InfHeader h;
    const int hst = md::gz::inf_header(f->in.data(), f->in.size(), &h);
    if (hst == MD_UNEXPECTED_END_OF_INPUT && !final) {  // not all there yet
      f->need = f->in.size() + 1;
      return false;
    }
    if (hst != MD_OK) return frame_fail(f, hst), false;
    f->in.erase(f->in.begin(), f->in.begin() + h.body);
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
inline void frame_took(InfFrame *f, uint32_t crc_piece, uint64_t len) {
  f->crc = f->total_out ? md::crc32_concat(f->crc, crc_piece, len) : crc_piece;
  f->total_out += len;
}
// the piece ended inside a block before the end of the input: what lies before that block went out, the input from the
// block boundary (bits from in[0], in_bit included) stays.  A new attempt only once input beyond the undecoded tail has
// arrived - that tail holds no complete block, decoding it again alone could not find one - and, when the piece held no
// block end at all, only once the buffered input has doubled (one long block fed in small pieces is decoded again a
// logarithmic number of times, not once per piece).
inline void frame_continue(InfFrame *f, uint64_t bits, uint32_t crc_piece, uint64_t len, uint32_t adler, size_t chunk) {
  const bool progress = bits > f->in_bit;
  frame_took(f, crc_piece, len);
  f->adler = adler;
  f->in.erase(f->in.begin(), f->in.begin() + (size_t)(bits >> 3));
  f->in_bit = (unsigned)(bits & 7);
  f->need = progress ? (f->in.size() + 1 > chunk ? f->in.size() + 1 : chunk) : (f->in.size() * 2 > chunk ? f->in.size() * 2 : chunk);
}
// the body ended (status MD_OK; `consumed` bytes of `in`) or failed with `st`; everything decoded went out, also in front
// of an error.  True when a trailer follows.
inline bool frame_body_end(InfFrame *f, int st, uint32_t crc_piece, uint64_t len, uint32_t sum, uint64_t consumed) {
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
// the trailer after the body: the stream ends here, or waits for the rest of the trailer (need).  GZip (Gz.Inf,
// lib/gz.ml:344-356): CRC-32 first, then ISIZE, little-endian; ZLIB (Zl.Inf, lib/zl.ml:171-186): the Adler-32, big-endian
inline void frame_trailer(InfFrame *f) {
  const size_t len = f->format == MD_FORMAT_GZIP ? 8 : 4;
  if (f->in.size() < len) {
    if (f->eoi) frame_fail(f, MD_UNEXPECTED_END_OF_INPUT);
    else f->need = len;
    return;
  }
  const uint8_t *t = f->in.data();
  f->status = MD_OK;
  if (f->format == MD_FORMAT_GZIP) {
    if (md::le32(t) != f->crc) frame_bad_checksum(f, md::le32(t), f->crc);
    else if (md::le32(t + 4) != (uint32_t)f->total_out) frame_bad_size(f, md::le32(t + 4), (uint32_t)f->total_out);
  } else if (md::be32(t) != f->checksum) {
    frame_bad_checksum(f, md::be32(t), f->checksum);
  }
  f->in.erase(f->in.begin(), f->in.begin() + len);
  f->finished = true;
}

#pragma GCC visibility pop
