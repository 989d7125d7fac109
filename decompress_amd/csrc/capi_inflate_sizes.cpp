// capi_inflate_sizes.cpp — the size query of the decoder (md_inflate_sizes_batch_*) and the output plan that follows it
// (md_inflate_plan_device): every stream's inflated size without decoding it, then offsets and capacities for
// md_inflate_batch_device, all on the device.
#include "ctx.hpp"

constexpr size_t kCountOrderFrom = 5121;  // 256 CUs x 20 resident wavefronts: smaller batches start all at once

int md_inflate_sizes_batch_device(md_ctx *ctx, int format, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                                  const uint64_t *d_in_len, uint64_t *d_out_len, uint64_t *d_consumed, int32_t *d_status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown format");
  if (n == 0) return MD_OK;
  if (n > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many streams in one batch");
  if (!d_in || !d_in_off || !d_in_len || !d_out_len || !d_consumed || !d_status)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "null array");
  MD_ON_DEVICE(ctx);
  const uint64_t *off = d_in_off, *len = d_in_len;
  int32_t *hstatus = nullptr;
  if (format == MD_FORMAT_GZIP) {  // header, the count kernel on the bodies, trailer (as md_inflate_batch_device)
    uint64_t *body_off = nullptr, *body_len = nullptr;
    const int rc = carve(ctx, ctx->gz_tmp, "hipMalloc(gzip scratch)", [&](md::Carver &c) {
      body_off = c.take<uint64_t>(n), body_len = c.take<uint64_t>(n);
      hstatus = c.take<int32_t>(n);
    });
    if (rc != MD_OK) return rc;
    MD_LAUNCH_TRY(ctx, md_launch_gz_header((uint32_t)n, d_in, d_in_off, d_in_len, body_off, body_len, hstatus, ctx->stream));
    off = body_off;
    len = body_len;
  }
  uint32_t *order = nullptr;
  const int orc = launch_order(ctx, n, kCountOrderFrom, &order);
  if (orc != MD_OK) return orc;
  uint64_t *dbg = ctx->dbg.as<uint64_t>();
  if (dbg) HIP_TRY(ctx, hipMemsetAsync(dbg, 0, 3 * 8, ctx->stream));
  MD_LAUNCH_TRY(ctx, md_launch_inflate_count(format == MD_FORMAT_GZIP ? MD_FORMAT_DEFLATE : format, (uint32_t)n, d_in, off, len, d_out_len, d_consumed,
                                             d_status, dbg, order, ctx->stream));
  if (format == MD_FORMAT_GZIP)
    MD_LAUNCH_TRY(ctx, md_launch_sizes_gz_finish((uint32_t)n, d_in, d_in_off, d_in_len, off, hstatus, d_out_len, d_consumed, d_status, ctx->stream));
  return MD_OK;
}

int md_inflate_sizes_batch_host(md_ctx *ctx, int format, size_t n, const uint8_t *h_in, size_t in_bytes, const uint64_t *in_off,
                                const uint64_t *in_len, uint64_t *out_len, uint64_t *consumed, int32_t *status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown format");
  if (n == 0) return MD_OK;
  if (!h_in || !in_off || !in_len || !out_len || !consumed || !status) return fail(ctx, MD_E_INVALID_ARGUMENT, "null array");
  uint64_t lo = in_bytes, hi = 0;  // the span of the caller's blob the streams lie in
  for (size_t i = 0; i < n; i++) {
    if (in_off[i] > in_bytes || in_len[i] > in_bytes - in_off[i])
      return fail(ctx, MD_E_INVALID_ARGUMENT, "input range out of bounds");
    if (in_len[i] > MD_MAX_INFLATE_IN) return fail(ctx, MD_E_INVALID_ARGUMENT, "stream longer than MD_MAX_INFLATE_IN");
    if (in_len[i]) {
      lo = in_off[i] < lo ? in_off[i] : lo;
      hi = in_off[i] + in_len[i] > hi ? in_off[i] + in_len[i] : hi;
    }
  }
  MD_ON_DEVICE(ctx);
  int rc = ctx->scratch[kHostIn].reserve(ctx, in_bytes + 64, "hipMalloc(host path input)");
  if (rc != MD_OK) return rc;
  uint8_t *din = (uint8_t *)ctx->scratch[kHostIn].p;
  uint64_t *d_in_off = nullptr, *d_in_len = nullptr, *d_out_len = nullptr, *d_consumed = nullptr;
  int32_t *dstatus = nullptr;
  rc = carve(ctx, ctx->scratch[kHostDesc], "hipMalloc(host path descriptors)", [&](md::Carver &c) {
    d_in_off = c.take<uint64_t>(n), d_in_len = c.take<uint64_t>(n), d_out_len = c.take<uint64_t>(n), d_consumed = c.take<uint64_t>(n);
    dstatus = c.take<int32_t>(n);
  });
  if (rc != MD_OK) return rc;
  hipStream_t st = ctx->stream;
  if (hi > lo) HIP_TRY(ctx, hipMemcpyAsync(din + lo, h_in + lo, hi - lo, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, md::to_device(d_in_off, in_off, n, st));
  HIP_TRY(ctx, md::to_device(d_in_len, in_len, n, st));
  rc = md_inflate_sizes_batch_device(ctx, format, n, din, d_in_off, d_in_len, d_out_len, d_consumed, dstatus);
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_host(out_len, d_out_len, n, st));
  HIP_TRY(ctx, md::to_host(consumed, d_consumed, n, st));
  HIP_TRY(ctx, md::to_host(status, dstatus, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return MD_OK;
}

int md_inflate_plan_device(md_ctx *ctx, size_t n, const uint64_t *d_out_len, size_t align, uint64_t *d_out_off,
                           uint64_t *d_out_cap, uint64_t *d_total) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (align == 0 || (align & (align - 1)) != 0) return fail(ctx, MD_E_INVALID_ARGUMENT, "align is not a power of two");
  if (!d_total || (n != 0 && (!d_out_len || !d_out_off || !d_out_cap))) return fail(ctx, MD_E_INVALID_ARGUMENT, "null array");
  MD_ON_DEVICE(ctx);
  MD_LAUNCH_TRY(ctx, md_launch_inflate_plan(n, d_out_len, align, d_out_off, d_out_cap, d_total, ctx->stream));
  return MD_OK;
}
