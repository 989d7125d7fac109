// capi_pack_write.cpp — writing a git pack (mdeflate.h: md_pack_delta_batch_device, md_pack_delta_batch_host,
// md_pack_write_bound, md_pack_write, md_pack_write_last).  The deltas are pack_write_kernels.hip's; names, payloads
// and CRCs are the batches the library has (md_sha1_batch_device, md_deflate_batch_device, md_launch_crc32); the distinct
// bases and their tables' places, the keep rule, the walk over offsets and headers and the trailer are the host's
// (pack_write.hpp).
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
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
  md::pkw::TablePlace at = {};
  for (size_t k = 0; k < n; k++) {
    const md_pack_delta_pair &p = in[by_base[k]];
    const bool fresh = k == 0 || in[by_base[k - 1]].base_off != p.base_off || in[by_base[k - 1]].base_len != p.base_len;
    if (fresh) at = plan->add_base(p.base_off, p.base_len);
    plan->pairs[by_base[k]] = DeltaPlan::pair(p, at);
  }
}

int enqueue_delta_plan(md_ctx *ctx, const DeltaPlan &plan, const uint8_t *d_src, DeltaKind kind, uint8_t *d_out, DeltaResults *res,
                       uint64_t *launches) {
  const size_t n = plan.pairs.size();
  hipStream_t st = ctx->stream;
  const bool carve_results = !res->out_len;
  md::pkw::Pair *d_pairs = nullptr;
  md::pkw::Base *d_bases = nullptr;
  int rc = carve(ctx, ctx->scratch[kPkwDesc], "hipMalloc(delta pairs)", [&](md::Carver &c) {
    d_pairs = c.take<md::pkw::Pair>(n), d_bases = c.take<md::pkw::Base>(plan.bases.size());
    if (carve_results) res->out_len = c.take<uint64_t>(n), res->status = c.take<int32_t>(n);
  });
  if (rc == MD_OK) rc = ctx->scratch[kPkwTables].reserve(ctx, (size_t)plan.room.words * 4, "hipMalloc(the bases' tables)");
  if (rc != MD_OK) return rc;
  uint32_t *tables = ctx->scratch[kPkwTables].as<uint32_t>();
  HIP_TRY(ctx, md::to_device(d_pairs, plan.pairs, st));
  HIP_TRY(ctx, md::to_device(d_bases, plan.bases, st));
  if (plan.room.words) HIP_TRY(ctx, hipMemsetAsync(tables, 0xff, (size_t)plan.room.words * 4, st));
  HIP_TRY(ctx, ctx->pkw_span.begin(st));
  if (plan.room.blocks) {
    MD_LAUNCH_TRY(ctx, md_launch_pkw_index((uint32_t)plan.bases.size(), plan.room.blocks, d_bases, d_src, tables, st));
    ++*launches;
  }
  if (kind == DeltaKind::kSizes) MD_LAUNCH_TRY(ctx, md_launch_pks_sizes((uint32_t)n, d_pairs, d_src, tables, res->out_len, res->status, st));
  else MD_LAUNCH_TRY(ctx, md_launch_pkw_delta((uint32_t)n, d_pairs, d_src, tables, d_out, res->out_len, res->status, st));
  ++*launches;
  HIP_TRY(ctx, ctx->pkw_span.end(st));
  return MD_OK;
}

namespace {

// the ranges of the pairs (host: against src_len, and out_off + out_cap against out_bytes)
int check_delta_pairs(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, bool host, size_t src_len, size_t out_bytes) {
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

}  // namespace

int delta_batch(md_ctx *ctx, bool host, DeltaKind kind, size_t n, const md_pack_delta_pair *pairs, const uint8_t *src, size_t src_len, uint8_t *out,
                size_t out_bytes, DeltaResults res) {
  if (n == 0) {
    ctx->pack_write_last = {};
    ctx->pkw_span.pending = false;
    return MD_OK;
  }
  if (n > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many pairs in one call");
  const bool sizes = kind == DeltaKind::kSizes;
  return no_bad_alloc(ctx, "host memory for the pairs", [&]() -> int {
    std::vector<md_pack_delta_pair> cleared;
    if (sizes) {  // the size calls do not look at out_off: cleared, it cannot fail the checks either
      cleared.assign(pairs, pairs + n);
      for (md_pack_delta_pair &p : cleared) p.out_off = 0;
      pairs = cleared.data(), out_bytes = SIZE_MAX;
    }
    int rc = check_delta_pairs(ctx, n, pairs, host, src_len, out_bytes);
    if (rc != MD_OK) return rc;
    uint64_t need = 0;  // of the host form's out
    if (host && !sizes)
      for (size_t i = 0; i < n; i++) need = std::max(need, pairs[i].out_off + pairs[i].out_cap);
    MD_ON_DEVICE(ctx);
    hipStream_t st = ctx->stream;
    DeltaResults d = res;
    if (host) {
      d = {};
      if ((rc = upload_host_in(ctx, src, src_len)) != MD_OK) return rc;
      src = ctx->scratch[kHostIn].as<uint8_t>();
      if (!sizes && (rc = ctx->scratch[kHostOut].reserve(ctx, (size_t)need + 64, "hipMalloc(host path output)")) != MD_OK) return rc;
    }
    uint8_t *d_out = host ? ctx->scratch[kHostOut].as<uint8_t>() : out;
    md_pack_write_stats stats = {};
    stats.pairs = n;
    DeltaPlan plan;
    plan_deltas(n, pairs, &plan);
    if ((rc = enqueue_delta_plan(ctx, plan, src, kind, d_out, &d, &stats.launches)) != MD_OK) return rc;
    if (host) {
      HIP_TRY(ctx, md::to_host(out, d_out, (size_t)need, st));
      HIP_TRY(ctx, md::to_host(res.out_len, d.out_len, n, st));
      HIP_TRY(ctx, md::to_host(res.status, d.status, n, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
      stats.delta_ns = ctx->pkw_span.ns();
    }
    ctx->pack_write_last = stats;
    ctx->pkw_span.pending = !host;
    return MD_OK;
  });
}

int md_pack_delta_batch_device(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *d_src, uint8_t *d_out, uint64_t *d_out_len,
                               int32_t *d_status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n && (!pairs || !d_src || !d_out || !d_out_len || !d_status)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_delta_batch_device: null pointer");
  return delta_batch(ctx, false, DeltaKind::kWrite, n, pairs, d_src, 0, d_out, 0, DeltaResults{d_out_len, d_status});
}

int md_pack_delta_batch_host(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *src, size_t src_len, uint8_t *out,
                             size_t out_bytes, uint64_t *out_len, int32_t *status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n && (!pairs || (!src && src_len) || (!out && out_bytes) || !out_len || !status)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_delta_batch_host: null pointer");
  return delta_batch(ctx, true, DeltaKind::kWrite, n, pairs, src, src_len, out, out_bytes, DeltaResults{out_len, status});
}

size_t md_pack_write_bound(size_t n, const md_pack_source *objs) {
  if (n && !objs) return 0;
  const uint64_t sum = md::pkw::write_bound(n, objs);
  return sum > SIZE_MAX ? 0 : (size_t)sum;
}

int check_sources(md_ctx *ctx, const char *who, size_t n, const md_pack_source *objs, size_t src_len) {
  for (size_t i = 0; i < n; i++) {
    const md_pack_source &o = objs[i];
    if (o.type < 1 || o.type > 4) return fail(ctx, MD_E_INVALID_ARGUMENT, (std::string(who) + ": a type is 1 .. 4").c_str());
    if (o.len > MD_MAX_STREAM || o.off > src_len || o.len > src_len - o.off)
      return fail(ctx, MD_E_INVALID_ARGUMENT, (std::string(who) + ": an object beyond the source, or too long").c_str());
  }
  return MD_OK;
}

namespace {

uint64_t round16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

void pack_header(size_t n, uint8_t h[12]) {
  const uint8_t bytes[12] = {'P', 'A', 'C', 'K', 0, 0, 0, 2, (uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n};
  memcpy(h, bytes, 12);
}

// the writer's device arrays of n objects, carved from one block
struct WriterDesc {
  uint64_t *off = nullptr, *len = nullptr, *pay_off = nullptr, *pay_len = nullptr, *slot_off = nullptr, *slot_cap = nullptr, *zlen = nullptr,
           *pk_len = nullptr, *pk_off = nullptr;
  int32_t *zstatus = nullptr;
  uint32_t *crc = nullptr;
  uint8_t *type = nullptr, *digest = nullptr, *head = nullptr, *head_len = nullptr;
  void carve(md::Carver *c, size_t n) {
    uint64_t **m64[8] = {&off, &len, &pay_off, &pay_len, &slot_off, &slot_cap, &zlen, &pk_len};
    for (uint64_t **p : m64) *p = c->take<uint64_t>(n);
    pk_off = c->take<uint64_t>(n + 1);
    zstatus = c->take<int32_t>(n);
    crc = c->take<uint32_t>(n);
    type = c->take<uint8_t>(n), digest = c->take<uint8_t>(n * kSha1Bytes);
    head = c->take<uint8_t>(n * md::pkw::kHeaderMax), head_len = c->take<uint8_t>(n);
  }
};

// One md_pack_write of n > 0 objects: what a step leaves for the steps behind it.  The steps run once, in the order they
// stand in, on the context's device; a host array that a step uploads from lives here or until that step has waited.
struct PackWriter {
  md_ctx *ctx;
  const size_t n;
  const md_pack_source *objs;
  md_pack_write_stats &stats;
  md_pack_write_result *res;
  WriterDesc d;
  uint8_t *d_in = nullptr, *slots = nullptr;  // the objects and behind them the deltas (kHostIn); the compressed payloads (kPkwSlots)
  std::vector<uint64_t> off, len, base;       // the objects as the launches and pack_write.hpp take them
  std::vector<uint8_t> type;
  std::vector<md_pack_delta_pair> pairs;  // the deltas that are tried: object i's is pairs[pair_of[i]] if tried[i]
  std::vector<uint64_t> pair_of, dl_len;  // (dl_len: per pair)
  std::vector<uint8_t> tried, keep;
  std::vector<uint64_t> pay_len, zlen;  // what object i is written from - its delta or its content -, and its stream's length
  std::vector<uint64_t> offset;         // where object i stands in the pack; offset[n]: the trailer
  std::vector<uint8_t> head, head_len;

  // Which deltas are tried, each with room behind the objects in kHostIn; returns the bytes of kHostIn.
  uint64_t try_pairs(bool deltas, size_t src_len) {
    off.resize(n), len.resize(n), base.resize(n), type.resize(n), tried.assign(n, 0), pair_of.assign(n, 0);
    const uint64_t deltas_at = round16(src_len);
    uint64_t room = 0;
    for (size_t i = 0; i < n; i++) {
      const md_pack_source &o = objs[i];
      off[i] = o.off, len[i] = o.len, type[i] = (uint8_t)o.type, base[i] = o.base;
      stats.payload_before += o.len;
      if (!deltas || o.base == MD_PACK_NO_BASE || !md::pkw::delta_tried(objs[o.base].len, o.len)) continue;
      tried[i] = 1, pair_of[i] = pairs.size();
      pairs.push_back(md_pack_delta_pair{objs[o.base].off, objs[o.base].len, o.off, o.len, deltas_at + room, md::pkw::delta_cap(o.len)});
      room += round16(pairs.back().out_cap);
    }
    return deltas_at + room;
  }

  // The objects to the device, and their names: ONE SHA-1 batch.
  int upload_and_name(const uint8_t *src, size_t src_len, uint64_t in_bytes) {
    hipStream_t st = ctx->stream;
    int rc = ctx->scratch[kHostIn].reserve(ctx, (size_t)in_bytes + 64, "hipMalloc(the objects and their deltas)");
    if (rc == MD_OK) rc = carve(ctx, ctx->scratch[kPkwObjs], "hipMalloc(the pack's objects)", [&](md::Carver &c) { d.carve(&c, n); });
    if (rc != MD_OK) return rc;
    d_in = ctx->scratch[kHostIn].as<uint8_t>();
    HIP_TRY(ctx, md::to_device(d_in, src, src_len, st));
    HIP_TRY(ctx, md::to_device(d.off, off, st));
    HIP_TRY(ctx, md::to_device(d.len, len, st));
    HIP_TRY(ctx, md::to_device(d.type, type, st));
    return md_sha1_batch_device(ctx, n, d_in, d.off, d.len, d.type, *std::max_element(len.begin(), len.end()), d.digest);
  }

  // The deltas, all pairs at once, and which of them are kept.
  int make_deltas(uint32_t max_depth) {
    hipStream_t st = ctx->stream;
    const size_t np = pairs.size();
    dl_len.assign(np, 0);
    std::vector<uint8_t> fitted(n, 0);
    if (np) {
      DeltaPlan plan;
      plan_deltas(np, pairs.data(), &plan);
      DeltaResults r;
      const int rc = enqueue_delta_plan(ctx, plan, d_in, DeltaKind::kWrite, d_in, &r, &stats.launches);
      if (rc != MD_OK) return rc;
      stats.pairs = np;
      std::vector<int32_t> dl_status(np);
      HIP_TRY(ctx, md::to_host(dl_len.data(), r.out_len, np, st));
      HIP_TRY(ctx, md::to_host(dl_status.data(), r.status, np, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
      stats.delta_ns = ctx->pkw_span.ns();
      for (size_t i = 0; i < n; i++) fitted[i] = tried[i] && dl_status[pair_of[i]] == MD_OK;
    }
    std::vector<uint32_t> depth(n);
    keep.resize(n);
    const md::pkw::Kept k = md::pkw::keep_rule(n, base.data(), tried.data(), fitted.data(), max_depth, keep.data(), depth.data());
    stats.kept = k.kept, stats.dropped_size = k.dropped_size, stats.dropped_depth = k.dropped_depth;
    res->deltas = k.kept;
    res->max_depth = *std::max_element(depth.begin(), depth.end());
    return MD_OK;
  }

  // The payloads - a kept delta, else the content - through ONE deflate batch into slots of their own.
  int deflate_payloads(int level) {
    hipStream_t st = ctx->stream;
    std::vector<uint64_t> pay_off(n), slot_off(n), slot_cap(n);
    std::vector<int32_t> zstatus(n);
    pay_len.resize(n), zlen.resize(n);
    uint64_t slots_bytes = 0;
    for (size_t i = 0; i < n; i++) {
      pay_off[i] = keep[i] ? pairs[pair_of[i]].out_off : off[i];
      pay_len[i] = keep[i] ? dl_len[pair_of[i]] : len[i];
      stats.payload_after += pay_len[i];
      slot_off[i] = slots_bytes, slot_cap[i] = md::pkw::stream_room(pay_len[i]);
      slots_bytes += round16(slot_cap[i]);
    }
    int rc = ctx->scratch[kPkwSlots].reserve(ctx, (size_t)slots_bytes + 64, "hipMalloc(the compressed payloads)");
    if (rc != MD_OK) return rc;
    slots = ctx->scratch[kPkwSlots].as<uint8_t>();
    HIP_TRY(ctx, md::to_device(d.pay_off, pay_off, st));
    HIP_TRY(ctx, md::to_device(d.pay_len, pay_len, st));
    HIP_TRY(ctx, md::to_device(d.slot_off, slot_off, st));
    HIP_TRY(ctx, md::to_device(d.slot_cap, slot_cap, st));
    const md_deflate_params p = gzip_body_params(level, (size_t)stats.payload_after);
    rc = md_deflate_batch_device(ctx, MD_FORMAT_ZLIB, &p, n, d_in, d.pay_off, d.pay_len, slots, d.slot_off, d.slot_cap, d.zlen, d.zstatus, nullptr);
    if (rc != MD_OK) return rc;
    HIP_TRY(ctx, md::to_host(zlen.data(), d.zlen, n, st));
    HIP_TRY(ctx, md::to_host(zstatus.data(), d.zstatus, n, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++)
      if (zstatus[i] != MD_OK) return fail(ctx, zstatus[i] == MD_UNEXPECTED_END_OF_OUTPUT ? MD_E_HIP : zstatus[i], "md_pack_write: a payload's stream failed (above its room?)");
    return MD_OK;
  }

  // Offsets and headers: the pack's length is known from here on, and whether it fits.
  int lay_out(size_t pack_cap, size_t *pack_len) {
    const std::vector<uint32_t> type32(type.begin(), type.end());
    offset.resize(n + 1), head.assign(n * md::pkw::kHeaderMax, 0), head_len.resize(n);
    md::pkw::walk_offsets(n, type32.data(), pay_len.data(), base.data(), keep.data(), zlen.data(), offset.data(), head.data(), head_len.data());
    const uint64_t total = offset[n] + md::pkw::kPackTrailer;
    if (total > SIZE_MAX) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_write: the pack does not fit size_t");
    *pack_len = (size_t)total;
    return total > pack_cap ? MD_UNEXPECTED_END_OF_OUTPUT : MD_OK;
  }

  // The pack assembled on the device, the CRC-32 of every packed object, and back: the pack, its trailer - one serial
  // message, the host's - and the idx's entries.
  int assemble(uint8_t *pack, md_pack_index_entry *entries) {
    hipStream_t st = ctx->stream;
    std::vector<uint64_t> pk_len(n);
    for (size_t i = 0; i < n; i++) pk_len[i] = offset[i + 1] - offset[i];
    const int rc = ctx->scratch[kHostOut].reserve(ctx, (size_t)(offset[n] + md::pkw::kPackTrailer) + 64, "hipMalloc(host path output)");
    if (rc != MD_OK) return rc;
    uint8_t *d_pack = ctx->scratch[kHostOut].as<uint8_t>();
    uint8_t head12[12];
    pack_header(n, head12);
    HIP_TRY(ctx, md::to_device(d.pk_off, offset, st));
    HIP_TRY(ctx, md::to_device(d.pk_len, pk_len, st));
    HIP_TRY(ctx, md::to_device(d.head, head, st));
    HIP_TRY(ctx, md::to_device(d.head_len, head_len, st));
    HIP_TRY(ctx, md::to_device(d_pack, head12, 12, st));
    MD_LAUNCH_TRY(ctx, md_launch_pkw_assemble((uint32_t)n, d.pk_off, d.head, d.head_len, slots, d.slot_off, d.zlen, d_pack, st));
    MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)n, d_pack, d.pk_off, d.pk_len, d.crc, st));
    stats.launches += 2;
    std::vector<uint32_t> crc(n);
    std::vector<uint8_t> digest(n * kSha1Bytes);
    HIP_TRY(ctx, md::to_host(pack, d_pack, (size_t)offset[n], st));
    HIP_TRY(ctx, md::to_host(crc.data(), d.crc, n, st));
    HIP_TRY(ctx, md::to_host(digest.data(), d.digest, digest.size(), st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    md::sha::sha1_of(pack, (size_t)offset[n], pack + offset[n]);
    for (size_t i = 0; i < n; i++) {
      entries[i].offset = offset[i], entries[i].crc32 = crc[i];
      memcpy(entries[i].name, &digest[i * kSha1Bytes], kSha1Bytes);
    }
    return MD_OK;
  }
};

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
  int rc = check_sources(ctx, "md_pack_write", n, objs, src_len);
  if (rc != MD_OK) return rc;
  for (size_t i = 0; i < n; i++)
    if (objs[i].base != MD_PACK_NO_BASE && (objs[i].base >= i || objs[objs[i].base].type != objs[i].type))
      return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_write: a base is an earlier object of the same type");
  ctx->pack_write_last = {};
  ctx->pkw_span.pending = false;
  res->n = n;
  if (n == 0) {  // the header and its SHA-1
    *pack_len = md::pkw::kPackHeader + md::pkw::kPackTrailer;
    if (pack_cap < *pack_len) return MD_UNEXPECTED_END_OF_OUTPUT;
    pack_header(0, pack);
    md::sha::sha1_of(pack, md::pkw::kPackHeader, pack + md::pkw::kPackHeader);
    return MD_OK;
  }
  return no_bad_alloc(ctx, "host memory for the pack's objects", [&]() -> int {
    PackWriter w{ctx, n, objs, ctx->pack_write_last, res};
    const uint64_t in_bytes = w.try_pairs(!(flags & MD_PACK_WRITE_NO_DELTA), src_len);
    MD_ON_DEVICE(ctx);
    int rc = w.upload_and_name(src, src_len, in_bytes);
    if (rc == MD_OK) rc = w.make_deltas(max_depth);
    if (rc == MD_OK) rc = w.deflate_payloads(level);
    if (rc == MD_OK) rc = w.lay_out(pack_cap, pack_len);
    if (rc == MD_OK) rc = w.assemble(pack, entries);
    return rc;
  });
}

int md_pack_write_last(const md_ctx *cctx, md_pack_write_stats *stats) {
  if (!cctx || !stats) return MD_E_INVALID_ARGUMENT;
  md_ctx *ctx = const_cast<md_ctx *>(cctx);  // (the device form's time is fetched when it is asked for)
  if (ctx->pkw_span.pending) {
    MD_ON_DEVICE(ctx);
    HIP_TRY(ctx, ctx->pkw_span.settle(&ctx->pack_write_last.delta_ns));
  }
  *stats = ctx->pack_write_last;
  return MD_OK;
}
