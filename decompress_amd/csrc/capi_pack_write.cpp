// capi_pack_write.cpp — writing a git pack (mdeflate.h: md_pack_delta_batch_device, md_pack_delta_batch_host,
// md_pack_write_bound, md_pack_write, md_pack_write_last).  The deltas are pack_write_kernels.hip's; names, payloads
// and CRCs are the batches the library has (md_sha1_batch_device, md_deflate_batch_device, md_launch_crc32); the distinct
// bases and their tables' places, the keep rule, the walk over offsets and headers and the trailer are the host's
// (pack_write.hpp).
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "pack_write.hpp"
#include "sha1_host.hpp"

void plan_deltas(size_t n, const md_pack_delta_pair *in, DeltaPlan *plan) {
  plan->pairs.resize(n);
  std::vector<uint32_t> by_base(n);
  for (size_t i = 0; i < n; i++) by_base[i] = (uint32_t)i;
  std::sort(by_base.begin(), by_base.end(), [&](uint32_t a, uint32_t b) {
    return in[a].base_off != in[b].base_off ? in[a].base_off < in[b].base_off : in[a].base_len < in[b].base_len;
  });
  for (size_t k = 0; k < n; k++) {
    const md_pack_delta_pair &p = in[by_base[k]];
    md::pkw::Pair &row = plan->pairs[by_base[k]];
    row.base_off = p.base_off, row.base_len = p.base_len, row.tgt_off = p.tgt_off, row.tgt_len = p.tgt_len;
    row.out_off = p.out_off, row.out_cap = p.out_cap, row.table_off = 0, row.bits = 0, row.reserved = 0;
    const uint64_t blocks = p.base_len / md::pkw::kBlock;
    if (blocks == 0) continue;
    const bool fresh = k == 0 || in[by_base[k - 1]].base_off != p.base_off || in[by_base[k - 1]].base_len != p.base_len;
    if (fresh) {
      md::pkw::Base b = {};
      b.off = p.base_off, b.table_off = plan->table_words, b.first_block = plan->blocks, b.bits = md::pkw::table_bits(blocks);
      plan->bases.push_back(b);
      plan->blocks += blocks;
      plan->table_words += (uint64_t)1 << b.bits;
    }
    row.table_off = plan->bases.back().table_off, row.bits = plan->bases.back().bits;
  }
}

int enqueue_delta_plan(md_ctx *ctx, const DeltaPlan &plan, const uint8_t *d_src, const std::function<void(md::Carver &)> &extra, const DeltaRun &run,
                       uint64_t *launches) {
  const size_t n = plan.pairs.size();
  hipStream_t st = ctx->stream;
  md::pkw::Pair *d_pairs = nullptr;
  md::pkw::Base *d_bases = nullptr;
  int rc = carve(ctx, ctx->scratch[kPkwDesc], "hipMalloc(delta pairs)", [&](md::Carver &c) {
    d_pairs = c.take<md::pkw::Pair>(n), d_bases = c.take<md::pkw::Base>(plan.bases.size());
    extra(c);
  });
  if (rc == MD_OK) rc = ctx->scratch[kPkwTables].reserve(ctx, (size_t)plan.table_words * 4, "hipMalloc(the bases' tables)");
  if (rc != MD_OK) return rc;
  uint32_t *tables = ctx->scratch[kPkwTables].as<uint32_t>();
  HIP_TRY(ctx, md::to_device(d_pairs, plan.pairs, st));
  HIP_TRY(ctx, md::to_device(d_bases, plan.bases, st));
  if (plan.table_words) HIP_TRY(ctx, hipMemsetAsync(tables, 0xff, (size_t)plan.table_words * 4, st));
  HIP_TRY(ctx, hipEventRecord(ctx->pkw_ev0, st));
  if (plan.blocks) {
    MD_LAUNCH_TRY(ctx, md_launch_pkw_index((uint32_t)plan.bases.size(), plan.blocks, d_bases, d_src, tables, st));
    ++*launches;
  }
  MD_LAUNCH_TRY(ctx, run(d_pairs, tables));
  ++*launches;
  HIP_TRY(ctx, hipEventRecord(ctx->pkw_ev1, st));
  return MD_OK;
}

uint64_t pkw_event_ns(md_ctx *ctx) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, ctx->pkw_ev0, ctx->pkw_ev1) != hipSuccess) ms = 0, (void)hipGetLastError();
  return (uint64_t)((double)ms * 1e6);
}

int check_delta_pairs(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, bool host, size_t src_len, size_t out_bytes) {
  if (n > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many pairs in one call");
  for (size_t i = 0; i < n; i++) {
    const md_pack_delta_pair &p = pairs[i];
    if (p.base_len > MD_MAX_STREAM || p.tgt_len > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "a base or target longer than MD_MAX_STREAM");
    if (p.base_off > UINT64_MAX - p.base_len || p.tgt_off > UINT64_MAX - p.tgt_len || p.out_off > UINT64_MAX - p.out_cap)
      return fail(ctx, MD_E_INVALID_ARGUMENT, "a range of a pair overflows");
    if (host && (p.base_off + p.base_len > src_len || p.tgt_off + p.tgt_len > src_len || p.out_off + p.out_cap > out_bytes))
      return fail(ctx, MD_E_INVALID_ARGUMENT, "a pair beyond its buffer");
  }
  return MD_OK;
}

namespace {

// the index launch and the delta launch between the context's two events, on its stream; `extra` carves what the caller
// wants from kPkwDesc beside the rows.  Nothing is read back.
template <class Extra>
int enqueue_deltas(md_ctx *ctx, const DeltaPlan &plan, const uint8_t *d_src, uint8_t *d_out, uint64_t **d_out_len, int32_t **d_status, Extra extra,
                   md_pack_write_stats *stats) {
  hipStream_t st = ctx->stream;
  const int rc = enqueue_delta_plan(ctx, plan, d_src, extra, [&](const md::pkw::Pair *d_pairs, const uint32_t *tables) {
    return md_launch_pkw_delta((uint32_t)plan.pairs.size(), d_pairs, d_src, tables, d_out, *d_out_len, *d_status, st);
  }, &stats->launches);
  if (rc != MD_OK) return rc;
  stats->pairs = plan.pairs.size();
  return MD_OK;
}

}  // namespace

int md_pack_delta_batch_device(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *d_src, uint8_t *d_out, uint64_t *d_out_len,
                               int32_t *d_status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->pack_write_last = {};
    ctx->pkw_pending = false;
    return MD_OK;
  }
  if (!pairs || !d_src || !d_out || !d_out_len || !d_status) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_delta_batch_device: null pointer");
  int rc = check_delta_pairs(ctx, n, pairs, false, 0, 0);
  if (rc != MD_OK) return rc;
  MD_ON_DEVICE(ctx);
  md_pack_write_stats stats = {};
  rc = no_bad_alloc(ctx, "host memory for the pairs", [&] {
    DeltaPlan plan;
    plan_deltas(n, pairs, &plan);
    return enqueue_deltas(ctx, plan, d_src, d_out, &d_out_len, &d_status, [](md::Carver &) {}, &stats);
  });
  if (rc != MD_OK) return rc;
  ctx->pack_write_last = stats;
  ctx->pkw_pending = true;
  return MD_OK;
}

int md_pack_delta_batch_host(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *src, size_t src_len, uint8_t *out,
                             size_t out_bytes, uint64_t *out_len, int32_t *status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->pack_write_last = {};
    ctx->pkw_pending = false;
    return MD_OK;
  }
  if (!pairs || (!src && src_len) || (!out && out_bytes) || !out_len || !status) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_delta_batch_host: null pointer");
  int rc = check_delta_pairs(ctx, n, pairs, true, src_len, out_bytes);
  if (rc != MD_OK) return rc;
  uint64_t need = 0;
  for (size_t i = 0; i < n; i++) need = std::max(need, pairs[i].out_off + pairs[i].out_cap);
  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  rc = upload_host_in(ctx, src, src_len);
  if (rc == MD_OK) rc = ctx->scratch[kHostOut].reserve(ctx, (size_t)need + 64, "hipMalloc(host path output)");
  if (rc != MD_OK) return rc;
  md_pack_write_stats stats = {};
  uint64_t *d_out_len = nullptr;
  int32_t *d_status = nullptr;
  rc = no_bad_alloc(ctx, "host memory for the pairs", [&] {
    DeltaPlan plan;
    plan_deltas(n, pairs, &plan);
    return enqueue_deltas(ctx, plan, ctx->scratch[kHostIn].as<uint8_t>(), ctx->scratch[kHostOut].as<uint8_t>(), &d_out_len, &d_status,
                          [&](md::Carver &c) { d_out_len = c.take<uint64_t>(n), d_status = c.take<int32_t>(n); }, &stats);
  });
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_host(out, ctx->scratch[kHostOut].as<uint8_t>(), (size_t)need, st));
  HIP_TRY(ctx, md::to_host(out_len, d_out_len, n, st));
  HIP_TRY(ctx, md::to_host(status, d_status, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  stats.delta_ns = pkw_event_ns(ctx);
  ctx->pack_write_last = stats;
  ctx->pkw_pending = false;
  return MD_OK;
}

size_t md_pack_write_bound(size_t n, const md_pack_source *objs) {
  if (n && !objs) return 0;
  const uint64_t sum = md::pkw::write_bound(n, objs);
  return sum > SIZE_MAX ? 0 : (size_t)sum;
}

namespace {

uint64_t round16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

int pack_write(md_ctx *ctx, int level, bool deltas, uint32_t max_depth, size_t n, const md_pack_source *objs, const uint8_t *src, size_t src_len,
               uint8_t *pack, size_t pack_cap, size_t *pack_len, md_pack_index_entry *entries, md_pack_write_result *res) {
  md_pack_write_stats &stats = ctx->pack_write_last;
  stats = {};
  ctx->pkw_pending = false;
  res->n = n;
  uint8_t head12[12] = {'P', 'A', 'C', 'K', 0, 0, 0, 2, (uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n};
  if (n == 0) {
    *pack_len = md::pkw::kPackHeader + md::pkw::kPackTrailer;
    if (pack_cap < *pack_len) return MD_UNEXPECTED_END_OF_OUTPUT;
    memcpy(pack, head12, 12);
    md::sha::Sha1 s;
    md::sha::sha1_init(&s);
    md::sha::sha1_update(&s, pack, 12);
    md::sha::sha1_final(&s, pack + 12);
    return MD_OK;
  }

  // -- the pairs: tried[i], its room behind the objects in kHostIn
  std::vector<uint8_t> tried(n, 0), fitted(n, 0), keep(n), h_type(n);
  std::vector<uint64_t> h_off(n), h_len(n), h_base(n), pair_of(n, 0);
  std::vector<md_pack_delta_pair> pairs;
  const uint64_t deltas_at = round16(src_len);
  uint64_t delta_room = 0, longest = 0;
  for (size_t i = 0; i < n; i++) {
    const md_pack_source &o = objs[i];
    h_off[i] = o.off, h_len[i] = o.len, h_type[i] = (uint8_t)o.type, h_base[i] = o.base;
    longest = std::max(longest, o.len);
    stats.payload_before += o.len;
    if (!deltas || o.base == MD_PACK_NO_BASE || !md::pkw::delta_tried(objs[o.base].len, o.len)) continue;
    tried[i] = 1, pair_of[i] = pairs.size();
    md_pack_delta_pair p = {objs[o.base].off, objs[o.base].len, o.off, o.len, deltas_at + delta_room, md::pkw::delta_cap(o.len)};
    pairs.push_back(p);
    delta_room += round16(p.out_cap);
  }
  const size_t np = pairs.size();

  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  int rc = ctx->scratch[kHostIn].reserve(ctx, (size_t)(deltas_at + delta_room) + 64, "hipMalloc(the objects and their deltas)");
  if (rc != MD_OK) return rc;
  uint8_t *d_in = ctx->scratch[kHostIn].as<uint8_t>();
  HIP_TRY(ctx, md::to_device(d_in, src, src_len, st));
  uint64_t *d_off = nullptr, *d_len = nullptr, *pay_off = nullptr, *pay_len = nullptr, *slot_off = nullptr, *slot_cap = nullptr, *zlen = nullptr,
           *pk_off = nullptr, *pk_len = nullptr, *dl_len = nullptr;
  int32_t *zstatus = nullptr, *dl_status = nullptr;
  uint32_t *crc = nullptr;
  uint8_t *d_type = nullptr, *digest = nullptr, *head = nullptr, *head_len = nullptr;
  rc = carve(ctx, ctx->scratch[kPkwObjs], "hipMalloc(the pack's objects)", [&](md::Carver &c) {
    d_off = c.take<uint64_t>(n), d_len = c.take<uint64_t>(n), pay_off = c.take<uint64_t>(n), pay_len = c.take<uint64_t>(n);
    slot_off = c.take<uint64_t>(n), slot_cap = c.take<uint64_t>(n), zlen = c.take<uint64_t>(n);
    pk_off = c.take<uint64_t>(n + 1), pk_len = c.take<uint64_t>(n), dl_len = c.take<uint64_t>(np);
    zstatus = c.take<int32_t>(n), dl_status = c.take<int32_t>(np);
    crc = c.take<uint32_t>(n);
    d_type = c.take<uint8_t>(n), digest = c.take<uint8_t>(n * kSha1Bytes);
    head = c.take<uint8_t>(n * md::pkw::kHeaderMax), head_len = c.take<uint8_t>(n);
  });
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_device(d_off, h_off, st));
  HIP_TRY(ctx, md::to_device(d_len, h_len, st));
  HIP_TRY(ctx, md::to_device(d_type, h_type, st));

  // -- names
  if ((rc = md_sha1_batch_device(ctx, n, d_in, d_off, d_len, d_type, longest, digest)) != MD_OK) return rc;

  // -- deltas, all pairs at once; which are kept
  std::vector<uint64_t> h_dl_len(np);
  std::vector<int32_t> h_dl_status(np);
  if (np) {
    DeltaPlan plan;
    plan_deltas(np, pairs.data(), &plan);
    if ((rc = enqueue_deltas(ctx, plan, d_in, d_in, &dl_len, &dl_status, [](md::Carver &) {}, &stats)) != MD_OK) return rc;
    HIP_TRY(ctx, md::to_host(h_dl_len.data(), dl_len, np, st));
    HIP_TRY(ctx, md::to_host(h_dl_status.data(), dl_status, np, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    stats.delta_ns = pkw_event_ns(ctx);
    for (size_t i = 0; i < n; i++) fitted[i] = tried[i] && h_dl_status[pair_of[i]] == MD_OK;
  }
  std::vector<uint32_t> depth(n), h_type32(n);
  const md::pkw::Kept k = md::pkw::keep_rule(n, h_base.data(), tried.data(), fitted.data(), max_depth, keep.data(), depth.data());
  stats.kept = k.kept, stats.dropped_size = k.dropped_size, stats.dropped_depth = k.dropped_depth;
  res->deltas = k.kept;

  // -- payloads: ONE deflate batch
  std::vector<uint64_t> h_pay_off(n), h_pay_len(n), h_slot_off(n), h_slot_cap(n), h_zlen(n);
  std::vector<int32_t> h_zstatus(n);
  uint64_t slots_bytes = 0;
  for (size_t i = 0; i < n; i++) {
    h_type32[i] = h_type[i];
    res->max_depth = std::max<uint64_t>(res->max_depth, depth[i]);
    h_pay_off[i] = keep[i] ? pairs[pair_of[i]].out_off : h_off[i];
    h_pay_len[i] = keep[i] ? h_dl_len[pair_of[i]] : h_len[i];
    stats.payload_after += h_pay_len[i];
    h_slot_off[i] = slots_bytes, h_slot_cap[i] = md::pkw::stream_room(h_pay_len[i]);
    slots_bytes += round16(h_slot_cap[i]);
  }
  rc = ctx->scratch[kPkwSlots].reserve(ctx, (size_t)slots_bytes + 64, "hipMalloc(the compressed payloads)");
  if (rc != MD_OK) return rc;
  uint8_t *slots = ctx->scratch[kPkwSlots].as<uint8_t>();
  HIP_TRY(ctx, md::to_device(pay_off, h_pay_off, st));
  HIP_TRY(ctx, md::to_device(pay_len, h_pay_len, st));
  HIP_TRY(ctx, md::to_device(slot_off, h_slot_off, st));
  HIP_TRY(ctx, md::to_device(slot_cap, h_slot_cap, st));
  const md_deflate_params p = gzip_body_params(level, (size_t)stats.payload_after);
  rc = md_deflate_batch_device(ctx, MD_FORMAT_ZLIB, &p, n, d_in, pay_off, pay_len, slots, slot_off, slot_cap, zlen, zstatus, nullptr);
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_host(h_zlen.data(), zlen, n, st));
  HIP_TRY(ctx, md::to_host(h_zstatus.data(), zstatus, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (size_t i = 0; i < n; i++)
    if (h_zstatus[i] != MD_OK) return fail(ctx, h_zstatus[i] == MD_UNEXPECTED_END_OF_OUTPUT ? MD_E_HIP : h_zstatus[i], "md_pack_write: a payload's stream failed (above its room?)");

  // -- offsets and headers, then the pack on the device
  std::vector<uint64_t> offset(n + 1), h_pk_len(n);
  std::vector<uint8_t> h_head(n * md::pkw::kHeaderMax, 0), h_head_len(n);
  md::pkw::walk_offsets(n, h_type32.data(), h_pay_len.data(), h_base.data(), keep.data(), h_zlen.data(), offset.data(), h_head.data(), h_head_len.data());
  const uint64_t total = offset[n] + md::pkw::kPackTrailer;
  if (total > SIZE_MAX) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_write: the pack does not fit size_t");
  *pack_len = (size_t)total;
  if (total > pack_cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  for (size_t i = 0; i < n; i++) h_pk_len[i] = offset[i + 1] - offset[i];
  rc = ctx->scratch[kHostOut].reserve(ctx, (size_t)total + 64, "hipMalloc(host path output)");
  if (rc != MD_OK) return rc;
  uint8_t *d_pack = ctx->scratch[kHostOut].as<uint8_t>();
  HIP_TRY(ctx, md::to_device(pk_off, offset, st));
  HIP_TRY(ctx, md::to_device(pk_len, h_pk_len, st));
  HIP_TRY(ctx, md::to_device(head, h_head, st));
  HIP_TRY(ctx, md::to_device(head_len, h_head_len, st));
  HIP_TRY(ctx, md::to_device(d_pack, head12, 12, st));
  MD_LAUNCH_TRY(ctx, md_launch_pkw_assemble((uint32_t)n, pk_off, head, head_len, slots, slot_off, zlen, d_pack, st));
  MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)n, d_pack, pk_off, pk_len, crc, st));
  stats.launches += 2;
  std::vector<uint32_t> h_crc(n);
  std::vector<uint8_t> h_digest(n * kSha1Bytes);
  HIP_TRY(ctx, md::to_host(pack, d_pack, (size_t)offset[n], st));
  HIP_TRY(ctx, md::to_host(h_crc.data(), crc, n, st));
  HIP_TRY(ctx, md::to_host(h_digest.data(), digest, h_digest.size(), st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  {  // the trailer: one serial message, the host's
    md::sha::Sha1 s;
    md::sha::sha1_init(&s);
    md::sha::sha1_update(&s, pack, (size_t)offset[n]);
    md::sha::sha1_final(&s, pack + offset[n]);
  }
  for (size_t i = 0; i < n; i++) {
    entries[i].offset = offset[i], entries[i].crc32 = h_crc[i];
    memcpy(entries[i].name, &h_digest[i * kSha1Bytes], kSha1Bytes);
  }
  return MD_OK;
}

}  // namespace

int md_pack_write(md_ctx *ctx, int level, unsigned flags, uint32_t max_depth, size_t n, const md_pack_source *objs, const uint8_t *src, size_t src_len,
                  uint8_t *pack, size_t pack_cap, size_t *pack_len, md_pack_index_entry *entries, md_pack_write_result *res) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!pack_len || !res || (n && (!objs || !entries)) || (!src && src_len) || (!pack && pack_cap)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_write: null pointer");
  *pack_len = 0;
  memset(res, 0, sizeof *res);
  if (flags & ~MD_PACK_WRITE_NO_DELTA) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_write: unknown flag");
  if (level < 0 || level > 9) return fail(ctx, MD_E_INVALID_ARGUMENT, "Invalid level of compression");
  if (n > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_write: too many objects in one call");
  for (size_t i = 0; i < n; i++) {
    const md_pack_source &o = objs[i];
    if (o.type < 1 || o.type > 4) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_write: a type is 1 .. 4");
    if (o.len > MD_MAX_STREAM || o.off > src_len || o.len > src_len - o.off) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_write: an object beyond the source, or too long");
    if (o.base != MD_PACK_NO_BASE && (o.base >= i || objs[o.base].type != o.type))
      return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_write: a base is an earlier object of the same type");
  }
  return no_bad_alloc(ctx, "host memory for the pack's objects", [&] {
    return pack_write(ctx, level, !(flags & MD_PACK_WRITE_NO_DELTA), max_depth, n, objs, src, src_len, pack, pack_cap, pack_len, entries, res);
  });
}

int md_pack_write_last(const md_ctx *cctx, md_pack_write_stats *stats) {
  if (!cctx || !stats) return MD_E_INVALID_ARGUMENT;
  md_ctx *ctx = const_cast<md_ctx *>(cctx);  // (the device form's time is fetched when it is asked for)
  if (ctx->pkw_pending) {
    MD_ON_DEVICE(ctx);
    HIP_TRY(ctx, hipEventSynchronize(ctx->pkw_ev1));
    ctx->pack_write_last.delta_ns = pkw_event_ns(ctx);
    ctx->pkw_pending = false;
  }
  *stats = ctx->pack_write_last;
  return MD_OK;
}
