// capi_lzo.cpp — md_lzo_*: batches on the device and the one-buffer calls.
#include "ctx.hpp"

static int lzo_batch_device(md_ctx *ctx, bool compress, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                            const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                            const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) return MD_OK;
  if (n > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many streams in one batch");
  if (!d_in_off || !d_in_len || !d_out_off || !d_out_cap || !d_out_len || !d_status)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "null descriptor array");
  MD_ON_DEVICE(ctx);
  // persistent workgroups (lzo_kernels.hip): as many as the chip holds at once, drawing streams from a counter
  const uint32_t slots = md_lzo_slots(compress ? 1 : 0, (uint32_t)ctx->cus);
  const size_t wgs = n < slots ? n : slots;
  if (compress) {  // Lzo's wrkmem: 16 K u16 entries per workgroup
    const int rc = ctx->lzo_ws.reserve(ctx, wgs * (size_t)(1u << 15), "hipMalloc(lzo wrkmem)");
    if (rc != MD_OK) return rc;
  }
  HIP_TRY(ctx, hipMemsetAsync(ctx->counters.as<uint32_t>(), 0, 4, ctx->stream));
  MD_LAUNCH_TRY(ctx, compress ? md_launch_lzo_compress((uint32_t)n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                                                       ctx->lzo_ws.as<uint16_t>(), ctx->counters.as<uint32_t>(), slots, ctx->stream)
                              : md_launch_lzo_uncompress((uint32_t)n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                                                         ctx->counters.as<uint32_t>(), slots, ctx->stream));
  return MD_OK;
}

int md_lzo_uncompress_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                                   const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                   const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status) {
  return lzo_batch_device(ctx, false, n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status);
}
int md_lzo_compress_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                                 const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                 const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status) {
  return lzo_batch_device(ctx, true, n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status);
}

static int lzo_one(md_ctx *ctx, bool compress, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                   size_t *written) {
  if (!ctx || !written || (!src && src_len) || (!dst && dst_cap)) return MD_E_INVALID_ARGUMENT;
  MD_ON_DEVICE(ctx);
  return one_through_batch(ctx, src, src_len, dst, dst_cap, written,
                           [&](const uint8_t *d_in, uint64_t *d64, uint8_t *d_out, int32_t *d_status, uint32_t *) {
                             return lzo_batch_device(ctx, compress, 1, d_in, d64, d64 + 1, d_out, d64 + 2, d64 + 3, d64 + 4, d_status);
                           });
}
int md_lzo_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                      size_t *written) {
  return lzo_one(ctx, false, src, src_len, dst, dst_cap, written);
}
int md_lzo_compress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                    size_t *written) {
  return lzo_one(ctx, true, src, src_len, dst, dst_cap, written);
}

// ---- sizes without decoding (lzo_count_kernel) and Lzo.uncompress_with_buffer on top of them ----

int md_lzo_sizes_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                              uint64_t *d_out_len, int32_t *d_status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) return MD_OK;
  if (n > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many streams in one batch");
  if (!d_in || !d_in_off || !d_in_len || !d_out_len || !d_status) return fail(ctx, MD_E_INVALID_ARGUMENT, "null array");
  MD_ON_DEVICE(ctx);
  const uint32_t slots = md_lzo_slots(2, (uint32_t)ctx->cus);
  HIP_TRY(ctx, hipMemsetAsync(ctx->counters.as<uint32_t>(), 0, 4, ctx->stream));
  MD_LAUNCH_TRY(ctx, md_launch_lzo_count((uint32_t)n, d_in, d_in_off, d_in_len, d_out_len, d_status, ctx->counters.as<uint32_t>(), slots, ctx->stream));
  return MD_OK;
}

int md_lzo_sizes_batch_host(md_ctx *ctx, size_t n, const uint8_t *h_in, size_t in_bytes, const uint64_t *in_off,
                            const uint64_t *in_len, uint64_t *out_len, int32_t *status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) return MD_OK;
  if (n > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many streams in one batch");
  if (!h_in || !in_off || !in_len || !out_len || !status) return fail(ctx, MD_E_INVALID_ARGUMENT, "null array");
  uint64_t lo = in_bytes, hi = 0;  // the span of the caller's blob the streams lie in
  for (size_t i = 0; i < n; i++) {
    if (in_off[i] > in_bytes || in_len[i] > in_bytes - in_off[i])
      return fail(ctx, MD_E_INVALID_ARGUMENT, "input range out of bounds");
    if (in_len[i] > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "stream longer than MD_MAX_STREAM");
    if (in_len[i]) {
      lo = in_off[i] < lo ? in_off[i] : lo;
      hi = in_off[i] + in_len[i] > hi ? in_off[i] + in_len[i] : hi;
    }
  }
  MD_ON_DEVICE(ctx);
  int rc = ctx->scratch[kHostIn].reserve(ctx, in_bytes + 64, "hipMalloc(host path input)");
  if (rc != MD_OK) return rc;
  uint8_t *din = (uint8_t *)ctx->scratch[kHostIn].p;
  uint64_t *d_in_off = nullptr, *d_in_len = nullptr, *d_out_len = nullptr;
  int32_t *dstatus = nullptr;
  rc = carve(ctx, ctx->scratch[kHostDesc], "hipMalloc(host path descriptors)", [&](md::Carver &c) {
    d_in_off = c.take<uint64_t>(n), d_in_len = c.take<uint64_t>(n), d_out_len = c.take<uint64_t>(n);
    dstatus = c.take<int32_t>(n);
  });
  if (rc != MD_OK) return rc;
  hipStream_t st = ctx->stream;
  if (hi > lo) HIP_TRY(ctx, hipMemcpyAsync(din + lo, h_in + lo, hi - lo, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, md::to_device(d_in_off, in_off, n, st));
  HIP_TRY(ctx, md::to_device(d_in_len, in_len, n, st));
  rc = md_lzo_sizes_batch_device(ctx, n, din, d_in_off, d_in_len, d_out_len, dstatus);
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_host(out_len, d_out_len, n, st));
  HIP_TRY(ctx, md::to_host(status, dstatus, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return MD_OK;
}

namespace {
struct HostBlock {  // a block of md_host_alloc that goes back unless it is handed to the caller
  md_ctx *ctx;
  void *p;
  ~HostBlock() { md_host_free(ctx, p); }
};
}  // namespace

int md_lzo_uncompress_with_buffer(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t **dst, size_t *dst_len) {
  if (!ctx || !dst || !dst_len) return MD_E_INVALID_ARGUMENT;
  *dst = nullptr;
  *dst_len = 0;
  if (!src && src_len) return fail(ctx, MD_E_INVALID_ARGUMENT, "null input");
  if (src_len > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "stream longer than MD_MAX_STREAM");
  MD_ON_DEVICE(ctx);
  md::DevBuf din, dout, ddesc;
  int rc = din.reserve(ctx, src_len + 16, "hipMalloc");
  if (rc == MD_OK) rc = ddesc.reserve(ctx, 6 * 8, "hipMalloc");
  if (rc != MD_OK) return rc;
  // in_off in_len out_off out_cap out_len, and the status right behind: size and status come back as one copy of 12 bytes
  uint64_t desc[5] = {0, src_len, 0, 0, 0};
  uint64_t *d64 = ddesc.as<uint64_t>();
  int32_t *dstatus = (int32_t *)(d64 + 5);
  struct {
    uint64_t len;
    int32_t status;
  } back = {0, 0};
  static_assert(sizeof(uint64_t) + sizeof(int32_t) == 12, "out_len and status: 12 bytes");
  hipStream_t st = ctx->stream;
  if (src_len) HIP_TRY(ctx, hipMemcpyAsync(din.p, src, src_len, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d64, desc, sizeof desc, hipMemcpyHostToDevice, st));
  rc = md_lzo_sizes_batch_device(ctx, 1, din.as<const uint8_t>(), d64, d64 + 1, d64 + 4, dstatus);
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(&back, d64 + 4, 12, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (back.status != MD_OK) return back.status;
  const uint64_t size = back.len;
  if (size > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "uncompressed size beyond MD_MAX_STREAM");
  HostBlock host = {ctx, md_host_alloc(ctx, (size_t)size)};
  if (!host.p) return MD_E_OUT_OF_MEMORY;
  rc = dout.reserve(ctx, (size_t)size + 16, "hipMalloc");
  if (rc != MD_OK) return rc;
  desc[3] = size;
  HIP_TRY(ctx, hipMemcpyAsync(d64 + 3, desc + 3, 8, hipMemcpyHostToDevice, st));
  rc = lzo_batch_device(ctx, false, 1, din.as<const uint8_t>(), d64, d64 + 1, dout.as<uint8_t>(), d64 + 2, d64 + 3, d64 + 4, dstatus);
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(&back, d64 + 4, 12, hipMemcpyDeviceToHost, st));
  if (size) HIP_TRY(ctx, hipMemcpyAsync(host.p, dout.p, (size_t)size, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  // the stream's status is the size call's: the decode can only agree with it
  if (back.status != MD_OK || back.len != size) return fail(ctx, MD_E_HIP, "lzo: the decode disagrees with the size call");
  *dst = (uint8_t *)host.p;
  *dst_len = (size_t)size;
  host.p = nullptr;
  return MD_OK;
}
