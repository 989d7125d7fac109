// capi_inflate.cpp — the decoder's entry points: batches on the device and from host buffers, a stream in pieces, and
// the one-stream calls that mirror the reference's.
#include <string.h>

#include <vector>

#include "ctx.hpp"
#include "gz_frame.hpp"
#include "host_pipeline.hpp"

constexpr size_t kOrderFrom = 2049;  // 256 CUs x 8 resident wavefronts: smaller batches start all at once

int md_inflate_batch_device(md_ctx *ctx, int format, size_t n, const uint8_t *d_in,
                            const uint64_t *d_in_off, const uint64_t *d_in_len, uint8_t *d_out,
                            const uint64_t *d_out_off, const uint64_t *d_out_cap,
                            uint64_t *d_out_len, uint64_t *d_consumed, int32_t *d_status,
                            uint32_t *d_checksum) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown format");
  if (n == 0) return MD_OK;
  if (n > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many streams in one batch");
  if (!d_in_off || !d_in_len || !d_out_off || !d_out_cap || !d_out_len || !d_consumed || !d_status)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "null descriptor array");
  MD_ON_DEVICE(ctx);
  if (format == MD_FORMAT_GZIP) {
    // Gz.Inf = header, De.Inf on the body, checksum (lib/gz.ml:463-531, :344-356)
    uint64_t *body_off = nullptr, *body_len = nullptr;
    int32_t *hstatus = nullptr;
    int rc = carve(ctx, ctx->gz_tmp, "hipMalloc(gzip scratch)", [&](md::Carver &c) {
      body_off = c.take<uint64_t>(n), body_len = c.take<uint64_t>(n);
      hstatus = c.take<int32_t>(n);
    });
    if (rc != MD_OK) return rc;
    MD_LAUNCH_TRY(ctx, md_launch_gz_header((uint32_t)n, d_in, d_in_off, d_in_len, body_off, body_len, hstatus, ctx->stream));
    rc = md_inflate_batch_device(ctx, MD_FORMAT_DEFLATE, n, d_in, body_off, body_len, d_out, d_out_off, d_out_cap,
                                 d_out_len, d_consumed, d_status, nullptr);
    if (rc != MD_OK) return rc;
    MD_LAUNCH_TRY(ctx, md_launch_gz_finish((uint32_t)n, d_in, d_in_off, d_in_len, body_off, hstatus, d_out, d_out_off, d_out_len, d_consumed, d_status,
                                           d_checksum, ctx->stream));
    return MD_OK;
  }
  // a batch of more streams than are resident at once (8 per CU) is started longest stream first; the scratch for the
  // order is kept and only ever grows (the one allocation a batch call can make, on its first large batch)
  uint32_t *order = nullptr;
  const int orc = launch_order(ctx, n, kOrderFrom, &order);
  if (orc != MD_OK) return orc;
  md::wv::InfArgs a{};
  a.format = format, a.n = (uint32_t)n;
  a.in = d_in, a.in_off = d_in_off, a.in_len = d_in_len;
  a.out = d_out, a.out_off = d_out_off, a.out_cap = d_out_cap;
  a.out_len = d_out_len, a.consumed = d_consumed, a.status = d_status, a.checksum = d_checksum;
  a.dbg = ctx->dbg.as<uint64_t>(), a.order = order, a.waves = ctx->inflate_waves;
  MD_LAUNCH_TRY(ctx, md_launch_inflate_wave(&a, ctx->stream));
  return MD_OK;
}

int md_inflate_batch_host(md_ctx *ctx, int format, size_t n, const uint8_t *h_in, size_t in_bytes,
                          const uint64_t *in_off, const uint64_t *in_len, uint8_t *h_out,
                          size_t out_bytes, const uint64_t *out_off, const uint64_t *out_cap,
                          uint64_t *out_len, uint64_t *consumed, int32_t *status,
                          uint32_t *checksum) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) return MD_OK;
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !consumed || !status)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "null descriptor array");
  for (size_t i = 0; i < n; i++) {
    if (in_off[i] > in_bytes || in_len[i] > in_bytes - in_off[i])
      return fail(ctx, MD_E_INVALID_ARGUMENT, "input range out of bounds");  // invalid_bounds, lib/de.ml:146
    if (in_len[i] > MD_MAX_INFLATE_IN) return fail(ctx, MD_E_INVALID_ARGUMENT, "stream longer than MD_MAX_INFLATE_IN");
    if (out_off[i] > out_bytes || out_cap[i] > out_bytes - out_off[i])
      return fail(ctx, MD_E_INVALID_ARGUMENT, "output range out of bounds");
  }
  MD_ON_DEVICE(ctx);
  ctx->par_last_pieces = ctx->par_last_rounds = 0;
  // A FEW LONG streams (a handful of big files): each of them in pieces, by the whole chip (inflate_parallel) - as streams
  // of a batch they would get one pair of wavefronts each.  What that path does not take, and the short streams beside
  // them, go through the batch as before.
  if (ctx->par_min && n <= 64) {
    std::vector<size_t> shorts, longs;
    // (each long stream is a call of ~1 ms at least, one after the other, where the batch kernel takes all n at once at ~0.2
    // GiB/s each: worth it from ~128 KiB of input per stream of the batch)
    const uint64_t long_from = ctx->par_min > n * ((uint64_t)128 << 10) ? ctx->par_min : n * ((uint64_t)128 << 10);
    for (size_t i = 0; i < n; i++) (in_len[i] >= long_from ? longs : shorts).push_back(i);
    if (!longs.empty()) {
      const size_t keep = ctx->par_min;
      // a batch of picked streams through this same entry point, the long-stream path switched off
      auto sub = [&](const std::vector<size_t> &pick) -> int {
        const size_t m = pick.size();
        std::vector<uint64_t> io(m), il(m), oo(m), oc(m), ol(m), cs(m);
        std::vector<int32_t> st(m);
        std::vector<uint32_t> ck(m);
        for (size_t k = 0; k < m; k++) {
          io[k] = in_off[pick[k]];
          il[k] = in_len[pick[k]];
          oo[k] = out_off[pick[k]];
          oc[k] = out_cap[pick[k]];
        }
        ctx->par_min = 0;
        const int rc = md_inflate_batch_host(ctx, format, m, h_in, in_bytes, io.data(), il.data(), h_out, out_bytes, oo.data(), oc.data(), ol.data(),
                                             cs.data(), st.data(), checksum ? ck.data() : nullptr);
        ctx->par_min = keep;
        if (rc != MD_OK) return rc;
        for (size_t k = 0; k < m; k++) {
          out_len[pick[k]] = ol[k];
          consumed[pick[k]] = cs[k];
          status[pick[k]] = st[k];
          if (checksum) checksum[pick[k]] = ck[k];
        }
        return MD_OK;
      };
      // the short ones first, as one batch (its copies take the span of the caller's blobs its streams lie in: what the long
      // streams' places receive from that is overwritten below)
      if (!shorts.empty()) {
        const int rc = sub(shorts);
        if (rc != MD_OK) return rc;
      }
      int pieces = 0, rounds = 0;
      for (size_t i : longs) {
        size_t used = 0, wrote = 0;
        uint32_t sum = 0;
        const int prc = inflate_parallel(ctx, format, h_in + in_off[i], (size_t)in_len[i], h_out + out_off[i], (size_t)out_cap[i], &used, &wrote,
                                         checksum ? &sum : nullptr);
        if (prc == MD_NOT_HANDLED) {  // (not a well-formed stream that fits: the batch path says what it is)
          const int rc = sub(std::vector<size_t>{i});
          if (rc != MD_OK) return rc;
          continue;
        }
        if (prc != MD_OK) return prc;
        out_len[i] = wrote;
        consumed[i] = used;
        status[i] = MD_OK;
        if (checksum) checksum[i] = sum;
        pieces += ctx->par_last_pieces;
        rounds = ctx->par_last_rounds > rounds ? ctx->par_last_rounds : rounds;
      }
      ctx->par_last_pieces = pieces;
      ctx->par_last_rounds = rounds;
      return MD_OK;
    }
  }
  int rc = ctx->scratch[kHostIn].reserve(ctx, in_bytes + 64, "hipMalloc(host path input)");
  if (rc == MD_OK) rc = ctx->scratch[kHostOut].reserve(ctx, out_bytes + 64, "hipMalloc(host path output)");
  if (rc != MD_OK) return rc;
  uint8_t *din = (uint8_t *)ctx->scratch[kHostIn].p, *dout = (uint8_t *)ctx->scratch[kHostOut].p;
  uint64_t *d_in_off = nullptr, *d_in_len = nullptr, *d_out_off = nullptr, *d_out_cap = nullptr, *d_out_len = nullptr, *d_consumed = nullptr;
  int32_t *dstatus = nullptr;
  uint32_t *dsum = nullptr;
  rc = carve(ctx, ctx->scratch[kHostDesc], "hipMalloc(host path descriptors)", [&](md::Carver &c) {
    d_in_off = c.take<uint64_t>(n), d_in_len = c.take<uint64_t>(n), d_out_off = c.take<uint64_t>(n), d_out_cap = c.take<uint64_t>(n);
    d_out_len = c.take<uint64_t>(n), d_consumed = c.take<uint64_t>(n);
    dstatus = c.take<int32_t>(n);
    dsum = c.take<uint32_t>(n);
  });
  if (rc != MD_OK) return rc;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, md::to_device(d_in_off, in_off, n, st));
  HIP_TRY(ctx, md::to_device(d_in_len, in_len, n, st));
  HIP_TRY(ctx, md::to_device(d_out_off, out_off, n, st));
  HIP_TRY(ctx, md::to_device(d_out_cap, out_cap, n, st));
  // a slice of 1 024 streams (4 per CU) runs at half the batch's rate per stream - still several times what the link to
  // the host moves (57 GB/s each way measured), so the copies stay the longer leg and more slices hide more of the kernels
  const std::vector<HostSlice> sl = host_slices(n, in_off, in_len, out_off, out_cap, 1024, (size_t)ctx->host_slices_max, in_bytes, out_bytes);
  rc = host_pipeline(ctx, sl, h_in, din, h_out, dout, [&](size_t i0, size_t cnt) {
    return md_inflate_batch_device(ctx, format, cnt, din, d_in_off + i0, d_in_len + i0, dout, d_out_off + i0, d_out_cap + i0, d_out_len + i0,
                                   d_consumed + i0, dstatus + i0, dsum + i0);
  });
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_host(out_len, d_out_len, n, st));
  HIP_TRY(ctx, md::to_host(consumed, d_consumed, n, st));
  HIP_TRY(ctx, md::to_host(status, dstatus, n, st));
  if (checksum) HIP_TRY(ctx, md::to_host(checksum, dsum, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return MD_OK;
}

// Pieces of n streams at once (mdeflate.h): the inflate kernel with its continuation arguments, descriptors in HBM.
int md_inflate_continue_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                                     const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                     const uint64_t *d_out_cap, const uint32_t *d_start_bit, const uint32_t *d_hist_len,
                                     const uint32_t *d_adler_in, uint64_t *d_out_len, uint64_t *d_consumed,
                                     int32_t *d_status, uint32_t *d_checksum, uint64_t *d_resume_bits,
                                     uint64_t *d_resume_out, uint32_t *d_resume_adler, uint32_t *d_resume_last) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) return MD_OK;
  if (n > 0xffffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many streams");
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_start_bit || !d_hist_len || !d_adler_in ||
      !d_out_len || !d_consumed || !d_status || !d_resume_bits || !d_resume_out || !d_resume_adler || !d_resume_last)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "null device pointer");
  MD_ON_DEVICE(ctx);
  uint32_t *order = nullptr;
  const int orc = launch_order(ctx, n, kOrderFrom, &order);
  if (orc != MD_OK) return orc;
  md::wv::InfArgs a{};
  a.format = MD_FORMAT_DEFLATE, a.n = (uint32_t)n;
  a.in = d_in, a.in_off = d_in_off, a.in_len = d_in_len;
  a.out = d_out, a.out_off = d_out_off, a.out_cap = d_out_cap;
  a.out_len = d_out_len, a.consumed = d_consumed, a.status = d_status, a.checksum = d_checksum;
  a.dbg = ctx->dbg.as<uint64_t>(), a.order = order, a.waves = ctx->inflate_waves;
  a.cont.start_bit = d_start_bit, a.cont.hist_len = d_hist_len, a.cont.adler_in = d_adler_in;
  a.cont.resume_bits = d_resume_bits, a.cont.resume_out = d_resume_out, a.cont.resume_adler = d_resume_adler, a.cont.resume_last = d_resume_last;
  MD_LAUNCH_TRY(ctx, md_launch_inflate_wave(&a, ctx->stream));
  return MD_OK;
}

// One piece of a raw DEFLATE stream that is decoded as it arrives (mdeflate.h): the inflate kernel on one stream with
// a starting bit, the window in front of the output buffer and the checksum state handed in, and the last block
// boundary inside the piece handed back.
int md_de_inf_continue_host(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, uint8_t *dst, size_t hist_len,
                            size_t dst_cap, uint32_t adler_in, unsigned flags, size_t *dst_len, int *status,
                            md_inf_resume *resume) {
  if (!ctx || (!src && src_len) || !dst || !dst_len || !status || !resume) return MD_E_INVALID_ARGUMENT;
  if (start_bit > 7 || hist_len > 32768 || hist_len > dst_cap || dst_cap > MD_MAX_STREAM || src_len > MD_MAX_INFLATE_IN)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "md_de_inf_continue_host: start_bit <= 7, hist_len <= 32768 and <= dst_cap");
  MD_ON_DEVICE(ctx);
  ctx->par_last_pieces = ctx->par_last_rounds = 0;
  if (ctx->par_min && src_len >= ctx->par_min) {  // a long piece: its complete blocks by the whole chip, the rest as before
    const int prc = continue_parallel(ctx, src, src_len, start_bit, dst, hist_len, dst_cap, adler_in, flags, dst_len, status, resume);
    if (prc != MD_NOT_HANDLED) return prc;
    ctx->par_last_pieces = 0;
  }
  return continue_serial(ctx, src, src_len, start_bit, dst, hist_len, dst_cap, adler_in, flags, dst_len, status, resume);
}
int inflate_piece(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, const uint8_t *hist, size_t hist_len, uint64_t room,
                  uint32_t adler_in, InfPiece *r) {
  // the context's scratch, grow-only: a long stream comes in many pieces, and three hipMalloc / hipFree per piece
  // cost more than a short piece's kernel
  md::DevBuf &din = ctx->scratch[kContIn], &dout = ctx->scratch[kContOut];
  int rc = din.reserve(ctx, src_len + 16, "hipMalloc(decoder piece input)");
  if (rc == MD_OK) rc = dout.reserve(ctx, hist_len + room + 16, "hipMalloc(decoder piece output)");
  if (rc != MD_OK) return rc;
  // descriptors: in_off in_len out_off out_cap out_len consumed resume_bits resume_out (u64); status, checksum,
  // start_bit, hist_len, adler_in, resume_adler, resume_last (u32)
  uint64_t h64[8] = {0, (uint64_t)src_len, 0, hist_len + room, 0, 0, 0, 0};
  uint32_t h32[7] = {0, 0, start_bit, (uint32_t)hist_len, adler_in, 0, 0};
  uint64_t *d64 = nullptr;
  uint32_t *d32 = nullptr;
  rc = carve(ctx, ctx->scratch[kContDesc], "hipMalloc(decoder piece descriptors)", [&](md::Carver &c) {
    d64 = c.take<uint64_t>(8);
    d32 = c.take<uint32_t>(7);
  });
  if (rc != MD_OK) return rc;
  hipStream_t st = ctx->stream;
  if (src_len) HIP_TRY(ctx, hipMemcpyAsync(din.p, src, src_len, hipMemcpyHostToDevice, st));
  if (hist_len) HIP_TRY(ctx, hipMemcpyAsync(dout.p, hist, hist_len, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d64, h64, sizeof h64, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d32, h32, sizeof h32, hipMemcpyHostToDevice, st));
  md::wv::InfArgs a{};  // (no profile, index order)
  a.format = MD_FORMAT_DEFLATE, a.n = 1;
  a.in = (const uint8_t *)din.p, a.in_off = d64 + 0, a.in_len = d64 + 1;
  a.out = (uint8_t *)dout.p, a.out_off = d64 + 2, a.out_cap = d64 + 3;
  a.out_len = d64 + 4, a.consumed = d64 + 5, a.status = (int32_t *)d32, a.checksum = d32 + 1;
  a.waves = ctx->inflate_waves;
  a.cont.start_bit = d32 + 2, a.cont.hist_len = d32 + 3, a.cont.adler_in = d32 + 4;
  a.cont.resume_bits = d64 + 6, a.cont.resume_out = d64 + 7, a.cont.resume_adler = d32 + 5, a.cont.resume_last = d32 + 6;
  MD_LAUNCH_TRY(ctx, md_launch_inflate_wave(&a, st));
  HIP_TRY(ctx, hipMemcpyAsync(h64, d64, sizeof h64, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(h32, d32, sizeof h32, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  *r = InfPiece{(int32_t)h32[0], h64[4], h64[5], h64[6], h64[7], h32[1], h32[5], h32[6]};
  return MD_OK;
}

int continue_serial(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, uint8_t *dst, size_t hist_len,
                    size_t dst_cap, uint32_t adler_in, unsigned flags, size_t *dst_len, int *status, md_inf_resume *resume) {
  InfPiece r;
  int rc = inflate_piece(ctx, src, src_len, start_bit, dst, hist_len, dst_cap - hist_len, adler_in, &r);
  if (rc != MD_OK) return rc;
  const uint8_t *d_out = ctx->scratch[kContOut].as<const uint8_t>();
  hipStream_t st = ctx->stream;
  const size_t produced = (size_t)r.out_len;
  if (produced > hist_len) HIP_TRY(ctx, hipMemcpy(dst + hist_len, d_out + hist_len, produced - hist_len, hipMemcpyDeviceToHost));
  *dst_len = produced;
  *status = r.status;
  resume->bits = r.resume_bits;
  resume->out = r.resume_out;
  resume->adler = r.resume_adler;
  resume->last = r.resume_last;
  resume->consumed = r.consumed;
  resume->checksum = r.checksum;
  resume->crc_out = resume->crc_end = 0;
  if (flags & MD_CONT_CRC32) {  // CRC-32 of the new output up to the block boundary, and up to where decoding got
    // (the piece's descriptors have been read: their block serves again)
    uint64_t *c64 = nullptr;
    uint32_t *c32 = nullptr;
    rc = carve(ctx, ctx->scratch[kContDesc], "hipMalloc(decoder piece descriptors)", [&](md::Carver &c) {
      c64 = c.take<uint64_t>(4);  // two offsets, two lengths
      c32 = c.take<uint32_t>(2);
    });
    if (rc != MD_OK) return rc;
    const uint64_t to_out = resume->out > hist_len ? resume->out - hist_len : 0, to_end = produced > hist_len ? produced - hist_len : 0;
    const uint64_t hc[4] = {(uint64_t)hist_len, (uint64_t)hist_len, to_out, to_end};
    uint32_t crc[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(c64, hc, sizeof hc, hipMemcpyHostToDevice, st));
    MD_LAUNCH_TRY(ctx, md_launch_crc32(2, d_out, c64, c64 + 2, c32, st));
    HIP_TRY(ctx, hipMemcpyAsync(crc, c32, sizeof crc, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    resume->crc_out = crc[0];
    resume->crc_end = crc[1];
  }
  return MD_OK;
}

static int inflate_one(md_ctx *ctx, int format, const uint8_t *src, size_t src_len, uint8_t *dst,
                       size_t dst_cap, size_t *consumed, size_t *written) {
  if (!ctx || !consumed || !written || (!src && src_len) || (!dst && dst_cap))
    return MD_E_INVALID_ARGUMENT;
  uint64_t in_off = 0, in_len = src_len, out_off = 0, out_cap = dst_cap, out_len = 0, used = 0;
  int32_t status = 0;
  int rc = md_inflate_batch_host(ctx, format, 1, src, src_len, &in_off, &in_len, dst, dst_cap,
                                 &out_off, &out_cap, &out_len, &used, &status, nullptr);
  if (rc != MD_OK) return rc;
  *consumed = (size_t)used;
  *written = (size_t)out_len;
  return status;
}

int md_de_inf_ns_inflate(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst,
                         size_t dst_cap, size_t *consumed, size_t *written) {
  return inflate_one(ctx, MD_FORMAT_DEFLATE, src, src_len, dst, dst_cap, consumed, written);
}

int md_zl_inf_ns_inflate(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst,
                         size_t dst_cap, size_t *consumed, size_t *written) {
  return inflate_one(ctx, MD_FORMAT_ZLIB, src, src_len, dst, dst_cap, consumed, written);
}


// De.Higher.uncompress / Zl.Higher.uncompress (lib/de.ml:4555-4571, lib/zl.ml:650-666): the whole stream in, the
// whole output out; the reference's `Error (`Msg s)` is md_status_string of the status returned
int md_de_higher_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *written) {
  size_t used = 0;
  return inflate_one(ctx, MD_FORMAT_DEFLATE, src, src_len, dst, dst_cap, &used, written);
}
int md_zl_higher_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *written) {
  size_t used = 0;
  return inflate_one(ctx, MD_FORMAT_ZLIB, src, src_len, dst, dst_cap, &used, written);
}

// The accessors of a finished Gz.Inf decoder (filename / comment / os / extra, lib/gz.ml:612-633):
// where the header fields sit in src.  Framing only — the kernels have validated the header.
static void gz_meta_of(const uint8_t *s, size_t n, md_gz_meta *m) {
  memset(m, 0, sizeof *m);
  md::gz::InfHeader h;
  if (md::gz::inf_header(s, n, &h) != MD_OK) return;
  m->flg = h.flg;
  m->mtime = h.mtime;
  m->xfl = h.xfl;
  m->os = h.os;
  m->has_extra = (h.flg & 4) != 0;
  m->extra_off = h.extra_off;
  m->extra_len = h.extra_len;
  m->has_name = (h.flg & 8) != 0;
  m->name_off = h.name_off;
  m->name_len = h.name_len;
  m->has_comment = (h.flg & 16) != 0;
  m->comment_off = h.comment_off;
  m->comment_len = h.comment_len;
}

int md_gz_higher_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                            size_t *consumed, size_t *written, md_gz_meta *meta) {
  int st = inflate_one(ctx, MD_FORMAT_GZIP, src, src_len, dst, dst_cap, consumed, written);
  if (meta) {
    memset(meta, 0, sizeof *meta);
    if (st == MD_OK) gz_meta_of(src, src_len, meta);
  }
  return st;
}
