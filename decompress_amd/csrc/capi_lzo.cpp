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
  const int e = compress ? md_launch_lzo_compress((uint32_t)n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                                  d_out_len, d_status, ctx->lzo_ws.as<uint16_t>(), ctx->counters.as<uint32_t>(), slots, ctx->stream)
                         : md_launch_lzo_uncompress((uint32_t)n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap,
                                                    d_out_len, d_status, ctx->counters.as<uint32_t>(), slots, ctx->stream);
  if (e != 0) return fail(ctx, MD_E_HIP, "lzo kernel launch", (hipError_t)e);
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
