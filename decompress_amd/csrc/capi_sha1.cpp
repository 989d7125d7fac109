// capi_sha1.cpp — SHA-1 of many buffers (mdeflate.h: md_sha1_batch_device, md_sha1_batch_host, md_sha1_last) and the hash
// pass that md_pack_read / md_pack_verify run for MD_PACK_VERIFY_NAME (sha1_enqueue), and the two trailers of a pack on the
// host (md_pack_check_trailers).  The kernel is sha1_kernels.hip; the header's formatter and the host's SHA-1 are
// sha1_host.hpp.
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "pack_index.hpp"
#include "sha1_host.hpp"

namespace {

// blocks of 64 bytes of a message of len bytes of content: header, content, 0x80 and the 64-bit length
uint64_t blocks_of(uint32_t type, uint64_t len) {
  uint32_t hw[md::sha::kHeaderWords];
  return (md::sha::git_header(type, (uint32_t)len, hw) + len + 9 + 63) >> 6;
}

int carve_batch(md_ctx *ctx, size_t n, Sha1Batch *b) {
  return carve(ctx, ctx->scratch[kShaDesc], "hipMalloc(SHA-1 descriptors)", [&](md::Carver &c) {
    b->off = c.take<uint64_t>(n), b->len = c.take<uint64_t>(n);
    b->state = c.take<md::sha::State>(n);
    b->index = c.take<uint32_t>(n), b->differs = c.take<uint32_t>(n);
    b->type = c.take<uint8_t>(n);
    b->digest = c.take<uint8_t>(n * kSha1Bytes), b->expect = c.take<uint8_t>(n * kSha1Bytes);
  });
}

}  // namespace

int sha1_enqueue(md_ctx *ctx, size_t n, const uint8_t *d_data, const uint64_t *off, const uint64_t *len, const uint8_t *type, Sha1Batch *b,
                 md_sha1_stats *stats) {
  if (n == 0) return MD_OK;
  int rc = carve_batch(ctx, n, b);
  if (rc != MD_OK) return rc;
  std::vector<uint64_t> blocks(n);
  std::vector<uint32_t> &order = b->order;
  order.resize(n);
  uint64_t sum = 0;
  for (size_t i = 0; i < n; i++) {
    blocks[i] = blocks_of(type ? type[i] : md::sha::kPlain, len[i]);
    order[i] = (uint32_t)i;
    sum += blocks[i];
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return blocks[x] > blocks[y]; });
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, md::to_device(b->off, off, n, st));
  HIP_TRY(ctx, md::to_device(b->len, len, n, st));
  HIP_TRY(ctx, md::to_device(b->index, order, st));
  if (type) HIP_TRY(ctx, md::to_device(b->type, type, n, st));
  md::sha::Args a = {};
  a.blocks = ctx->sha1_launch_blocks;
  a.data = d_data, a.off = b->off, a.len = b->len, a.type = type ? b->type : nullptr, a.index = b->index;
  a.state = b->state, a.digest = b->digest;
  // launch j takes the messages of more than j * blocks blocks: a prefix of the order, shrinking
  size_t active = n;
  for (uint64_t at = 0; at < blocks[order[0]]; at += a.blocks) {
    while (active && blocks[order[active - 1]] <= at) active--;
    a.count = (uint32_t)active;
    a.fresh = at == 0;
    MD_LAUNCH_TRY(ctx, md_launch_sha1(&a, st));
    stats->launches++;
  }
  stats->messages += n;
  stats->blocks += sum;
  return MD_OK;
}

int md_sha1_batch_host(md_ctx *ctx, size_t n, const uint8_t *data, size_t data_len, const uint64_t *off, const uint64_t *len,
                       const uint8_t *type, uint8_t *digest) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->sha1_last = {};
    ctx->sha1_span.pending = false;
    return MD_OK;
  }
  if (n > 0x7fffffffull || (!data && data_len) || !off || !len || !digest) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_sha1_batch_host: null pointer");
  for (size_t i = 0; i < n; i++) {
    if (len[i] > MD_MAX_STREAM || off[i] > data_len || len[i] > data_len - off[i])
      return fail(ctx, MD_E_INVALID_ARGUMENT, "md_sha1_batch_host: a message beyond the data, or longer than MD_MAX_STREAM");
    if (type && type[i] > md::sha::kMaxType) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_sha1_batch_host: a type above 4");
  }
  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  int rc = upload_host_in(ctx, data, data_len);
  if (rc != MD_OK) return rc;
  Sha1Batch b;
  md_sha1_stats stats = {};
  HIP_TRY(ctx, ctx->sha1_span.begin(st));
  rc = no_bad_alloc(ctx, "host memory for the batch's order",
                    [&] { return sha1_enqueue(ctx, n, ctx->scratch[kHostIn].as<uint8_t>(), off, len, type, &b, &stats); });
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, ctx->sha1_span.end(st));
  HIP_TRY(ctx, md::to_host(digest, b.digest, n * kSha1Bytes, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  stats.device_ns = ctx->sha1_span.ns();
  ctx->sha1_last = stats;
  ctx->sha1_span.pending = false;
  return MD_OK;
}

int md_sha1_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_data, const uint64_t *d_off, const uint64_t *d_len, const uint8_t *d_type,
                         uint64_t max_len, uint8_t *d_digest) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->sha1_last = {};
    ctx->sha1_span.pending = false;
    return MD_OK;
  }
  if (n > 0x7fffffffull || !d_off || !d_len || !d_digest || max_len > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "bad sha1 batch");
  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  md::sha::State *state = nullptr;
  const int rc = carve(ctx, ctx->scratch[kShaDesc], "hipMalloc(SHA-1 states)", [&](md::Carver &c) { state = c.take<md::sha::State>(n); });
  if (rc != MD_OK) return rc;
  md::sha::Args a = {};
  a.count = (uint32_t)n, a.blocks = ctx->sha1_launch_blocks;
  a.data = d_data, a.off = d_off, a.len = d_len, a.type = d_type, a.state = state, a.digest = d_digest;
  const uint64_t longest = blocks_of(1, max_len);  // (the longest header: a commit's)
  md_sha1_stats stats = {};
  HIP_TRY(ctx, ctx->sha1_span.begin(st));
  for (uint64_t at = 0; at < longest; at += a.blocks) {
    a.fresh = at == 0;
    MD_LAUNCH_TRY(ctx, md_launch_sha1(&a, st));
    stats.launches++;
  }
  HIP_TRY(ctx, ctx->sha1_span.end(st));
  stats.messages = n;  // (blocks: the lengths are the device's, the host has no count)
  ctx->sha1_last = stats;
  ctx->sha1_span.pending = true;
  return MD_OK;
}

int md_sha1_last(const md_ctx *cctx, md_sha1_stats *stats) {
  if (!cctx || !stats) return MD_E_INVALID_ARGUMENT;
  md_ctx *ctx = const_cast<md_ctx *>(cctx);  // (the device form's time is fetched when it is asked for)
  if (ctx->sha1_span.pending) {
    MD_ON_DEVICE(ctx);
    HIP_TRY(ctx, ctx->sha1_span.settle(&ctx->sha1_last.device_ns));
  }
  *stats = ctx->sha1_last;
  return MD_OK;
}

int md_pack_check_trailers(const uint8_t *pack, size_t pack_len, const uint8_t *idx, size_t idx_len, int *pack_ok, int *idx_ok) {
  if (!pack || !idx || !pack_ok || !idx_ok) return MD_E_INVALID_ARGUMENT;
  if (idx_len < 8 + 1024 + 40) return MD_INVALID_INDEX;
  if (pack_len < md::pack::kPackHeader + md::pack::kPackTrailer) return MD_INVALID_PACK;
  uint8_t digest[20];
  const struct {
    const uint8_t *p;
    size_t len;
    int *ok;
  } files[2] = {{pack, pack_len, pack_ok}, {idx, idx_len, idx_ok}};
  for (const auto &f : files) {
    md::sha::sha1_of(f.p, f.len - 20, digest);
    *f.ok = memcmp(digest, f.p + f.len - 20, 20) == 0;
  }
  return MD_OK;
}
