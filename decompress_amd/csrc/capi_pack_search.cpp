// capi_pack_search.cpp — choosing the bases of a pack's deltas (mdeflate.h: md_pack_sketch_device, md_pack_sketch_host,
// md_pack_delta_sizes_device, md_pack_delta_sizes_host, md_pack_choose_bases, md_pack_search_last).  The sketches and
// the count-only deltas are pack_search_kernels.hip's, the index of the candidates pack_write_kernels.hip's; the pack order, the
// groups of equal features and the choice are the host's (pack_search.hpp).
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "pack_search.hpp"

namespace {

uint64_t ns_since(std::chrono::steady_clock::time_point t0) {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}

// the segments of n objects, object i at off[i] with len[i] bytes; false: more than one launch strides over
bool cut_segments(size_t n, const uint64_t *off, const uint64_t *len, std::vector<md::pks::Seg> *segs) {
  uint64_t count = 0;
  for (size_t i = 0; i < n; i++) count += md::pks::segments(len[i]);
  if (count > md::pks::kMaxPairs) return false;
  segs->reserve((size_t)count);
  for (size_t i = 0; i < n; i++) {
    const uint64_t npos = md::pks::positions(len[i]);
    for (uint64_t p = 0; p < npos; p += md::pks::kSegPositions) {
      md::pks::Seg s;
      s.off = off[i] + p, s.npos = (uint32_t)std::min<uint64_t>(npos - p, md::pks::kSegPositions), s.obj = (uint32_t)i;
      segs->push_back(s);
    }
  }
  return true;
}

int check_objects(md_ctx *ctx, size_t n, const uint64_t *off, const uint64_t *len, bool host, size_t src_len) {
  if (n > md::pks::kMaxPairs) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many objects in one call");
  for (size_t i = 0; i < n; i++) {
    if (len[i] > MD_MAX_STREAM || off[i] > UINT64_MAX - len[i]) return fail(ctx, MD_E_INVALID_ARGUMENT, "an object longer than MD_MAX_STREAM, or a range that overflows");
    if (host && (off[i] > src_len || len[i] > src_len - off[i])) return fail(ctx, MD_E_INVALID_ARGUMENT, "an object beyond the source");
  }
  return MD_OK;
}

// features preset to all ones and the sketch launch between pkw_ev0 and pkw_ev1, on the context's stream.  d_features null:
// they are carved from kPkwDesc behind the segments (*features says where).  Nothing is read back.
int enqueue_sketch(md_ctx *ctx, size_t n, const std::vector<md::pks::Seg> &segs, const uint8_t *d_src, uint32_t *d_features, uint32_t **features,
                   uint64_t *launches) {
  hipStream_t st = ctx->stream;
  md::pks::Seg *d_segs = nullptr;
  uint32_t *carved = nullptr;
  const int rc = carve(ctx, ctx->scratch[kPkwDesc], "hipMalloc(the objects' segments)", [&](md::Carver &c) {
    d_segs = c.take<md::pks::Seg>(segs.size());
    if (!d_features) carved = c.take<uint32_t>(n * md::pks::kFeatures);
  });
  if (rc != MD_OK) return rc;
  *features = d_features ? d_features : carved;
  HIP_TRY(ctx, md::to_device(d_segs, segs, st));
  HIP_TRY(ctx, hipMemsetAsync(*features, 0xff, n * md::pks::kFeatures * sizeof(uint32_t), st));
  HIP_TRY(ctx, hipEventRecord(ctx->pkw_ev0, st));
  if (!segs.empty()) {
    MD_LAUNCH_TRY(ctx, md_launch_pks_sketch((uint32_t)segs.size(), d_segs, d_src, *features, st));
    ++*launches;
  }
  HIP_TRY(ctx, hipEventRecord(ctx->pkw_ev1, st));
  return MD_OK;
}

// the pairs with out_off cleared - the sizes' calls do not look at it - and checked as the delta batch checks them
int sized_pairs(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, bool host, size_t src_len, std::vector<md_pack_delta_pair> *out) {
  if (n > md::pks::kMaxPairs) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many pairs in one call");
  out->assign(pairs, pairs + n);
  for (md_pack_delta_pair &p : *out) p.out_off = 0;
  return check_delta_pairs(ctx, n, out->data(), host, src_len, SIZE_MAX);
}

// the index launch and the size launch over a plan
int enqueue_sizes(md_ctx *ctx, const DeltaPlan &plan, const uint8_t *d_src, uint64_t **d_out_len, int32_t **d_status, bool carve_results,
                  uint64_t *launches) {
  const size_t n = plan.pairs.size();
  hipStream_t st = ctx->stream;
  return enqueue_delta_plan(
      ctx, plan, d_src,
      [&](md::Carver &c) {
        if (carve_results) *d_out_len = c.take<uint64_t>(n), *d_status = c.take<int32_t>(n);
      },
      [&](const md::pkw::Pair *d_pairs, const uint32_t *tables) { return md_launch_pks_sizes((uint32_t)n, d_pairs, d_src, tables, *d_out_len, *d_status, st); },
      launches);
}

}  // namespace

int md_pack_sketch_device(md_ctx *ctx, size_t n, const uint64_t *off, const uint64_t *len, const uint8_t *d_src, uint32_t *d_features) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) return MD_OK;
  if (!off || !len || !d_src || !d_features) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_sketch_device: null pointer");
  int rc = check_objects(ctx, n, off, len, false, 0);
  if (rc != MD_OK) return rc;
  MD_ON_DEVICE(ctx);
  return no_bad_alloc(ctx, "host memory for the segments", [&]() -> int {
    std::vector<md::pks::Seg> segs;
    if (!cut_segments(n, off, len, &segs)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_sketch_device: too many segments in one call");
    uint32_t *features = nullptr;
    uint64_t launches = 0;
    return enqueue_sketch(ctx, n, segs, d_src, d_features, &features, &launches);
  });
}

int md_pack_sketch_host(md_ctx *ctx, size_t n, const uint64_t *off, const uint64_t *len, const uint8_t *src, size_t src_len, uint32_t *features) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) return MD_OK;
  if (!off || !len || (!src && src_len) || !features) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_sketch_host: null pointer");
  int rc = check_objects(ctx, n, off, len, true, src_len);
  if (rc != MD_OK) return rc;
  MD_ON_DEVICE(ctx);
  if ((rc = upload_host_in(ctx, src, src_len)) != MD_OK) return rc;
  uint32_t *d_features = nullptr;
  rc = no_bad_alloc(ctx, "host memory for the segments", [&]() -> int {
    std::vector<md::pks::Seg> segs;
    if (!cut_segments(n, off, len, &segs)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_sketch_host: too many segments in one call");
    uint64_t launches = 0;
    return enqueue_sketch(ctx, n, segs, ctx->scratch[kHostIn].as<uint8_t>(), nullptr, &d_features, &launches);
  });
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_host(features, d_features, n * md::pks::kFeatures, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MD_OK;
}

int md_pack_delta_sizes_device(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *d_src, uint64_t *d_out_len, int32_t *d_status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->pack_write_last = {};
    ctx->pkw_pending = false;
    return MD_OK;
  }
  if (!pairs || !d_src || !d_out_len || !d_status) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_delta_sizes_device: null pointer");
  md_pack_write_stats stats = {};
  const int rc = no_bad_alloc(ctx, "host memory for the pairs", [&]() -> int {
    std::vector<md_pack_delta_pair> rows;
    int rc = sized_pairs(ctx, n, pairs, false, 0, &rows);
    if (rc != MD_OK) return rc;
    MD_ON_DEVICE(ctx);
    DeltaPlan plan;
    plan_deltas(n, rows.data(), &plan);
    return enqueue_sizes(ctx, plan, d_src, &d_out_len, &d_status, false, &stats.launches);
  });
  if (rc != MD_OK) return rc;
  stats.pairs = n;
  ctx->pack_write_last = stats;
  ctx->pkw_pending = true;
  return MD_OK;
}

int md_pack_delta_sizes_host(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *src, size_t src_len, uint64_t *out_len,
                             int32_t *status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->pack_write_last = {};
    ctx->pkw_pending = false;
    return MD_OK;
  }
  if (!pairs || (!src && src_len) || !out_len || !status) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_delta_sizes_host: null pointer");
  md_pack_write_stats stats = {};
  const int rc = no_bad_alloc(ctx, "host memory for the pairs", [&]() -> int {
    std::vector<md_pack_delta_pair> rows;
    int rc = sized_pairs(ctx, n, pairs, true, src_len, &rows);
    if (rc != MD_OK) return rc;
    MD_ON_DEVICE(ctx);
    hipStream_t st = ctx->stream;
    if ((rc = upload_host_in(ctx, src, src_len)) != MD_OK) return rc;
    DeltaPlan plan;
    plan_deltas(n, rows.data(), &plan);
    uint64_t *d_out_len = nullptr;
    int32_t *d_status = nullptr;
    if ((rc = enqueue_sizes(ctx, plan, ctx->scratch[kHostIn].as<uint8_t>(), &d_out_len, &d_status, true, &stats.launches)) != MD_OK) return rc;
    HIP_TRY(ctx, md::to_host(out_len, d_out_len, n, st));
    HIP_TRY(ctx, md::to_host(status, d_status, n, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return MD_OK;
  });
  if (rc != MD_OK) return rc;
  stats.pairs = n;
  stats.delta_ns = pkw_event_ns(ctx);
  ctx->pack_write_last = stats;
  ctx->pkw_pending = false;
  return MD_OK;
}

namespace {

int choose_bases(md_ctx *ctx, uint32_t window, uint32_t max_depth, size_t n, const md_pack_source *objs, const uint8_t *src, size_t src_len,
                 md_pack_source *sorted, uint64_t *order) {
  md_pack_search_stats &stats = ctx->pack_search_last;
  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  int rc = upload_host_in(ctx, src, src_len);
  if (rc != MD_OK) return rc;
  const uint8_t *d_src = ctx->scratch[kHostIn].as<uint8_t>();

  // -- sketches
  std::vector<uint64_t> off(n), len(n);
  for (size_t i = 0; i < n; i++) off[i] = objs[i].off, len[i] = objs[i].len, stats.featured += md::pks::has_features(objs[i].len);
  std::vector<md::pks::Seg> segs;
  if (!cut_segments(n, off.data(), len.data(), &segs)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_choose_bases: too many segments in one call");
  uint32_t *d_features = nullptr;
  if ((rc = enqueue_sketch(ctx, n, segs, d_src, nullptr, &d_features, &stats.launches)) != MD_OK) return rc;
  std::vector<uint32_t> features(n * md::pks::kFeatures);
  HIP_TRY(ctx, md::to_host(features.data(), d_features, features.size(), st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  stats.sketch_ns = pkw_event_ns(ctx);

  // -- pack order and candidates
  auto t0 = std::chrono::steady_clock::now();
  md::pks::pack_order(n, objs, order);
  md::pks::Pairs cand;
  md::pks::candidates(n, objs, order, features.data(), window, &cand);
  const size_t np = cand.base.size();
  stats.pairs = np;
  // the plan: the distinct bases are the ranks that are some pair's base, their tables in rank order (plan_deltas would sort
  // the pairs by base to find them; here the ranks say it)
  DeltaPlan plan;
  plan.pairs.resize(np);
  std::vector<uint32_t> base_at(n, UINT32_MAX);
  for (size_t k = 0; k < np; k++) base_at[cand.base[k]] = 0;
  for (size_t r = 0; r < n; r++) {
    if (base_at[r] == UINT32_MAX) continue;
    const md_pack_source &o = objs[order[r]];
    const uint64_t blocks = o.len / md::pkw::kBlock;  // (at least one: a candidate has features)
    md::pkw::Base b = {};
    b.off = o.off, b.table_off = plan.table_words, b.first_block = plan.blocks, b.bits = md::pkw::table_bits(blocks);
    base_at[r] = (uint32_t)plan.bases.size();
    plan.bases.push_back(b);
    plan.blocks += blocks;
    plan.table_words += (uint64_t)1 << b.bits;
  }
  for (size_t t = 0; t < n; t++) {
    const md_pack_source &o = objs[order[t]];
    for (uint64_t k = cand.first[t]; k < cand.first[t + 1]; k++) {
      const md_pack_source &b = objs[order[cand.base[k]]];
      const md::pkw::Base &tb = plan.bases[base_at[cand.base[k]]];
      plan.pairs[k] = {b.off, b.len, o.off, o.len, 0, md::pkw::delta_cap(o.len), tb.table_off, tb.bits, 0};
    }
  }
  stats.host_ns = ns_since(t0);

  // -- scores: one index launch over the distinct candidates, one size launch over the pairs
  std::vector<uint64_t> dl_len(np);
  std::vector<int32_t> dl_status(np);
  std::vector<uint8_t> fitted(np);
  if (np) {
    uint64_t *d_len = nullptr;
    int32_t *d_status = nullptr;
    if ((rc = enqueue_sizes(ctx, plan, d_src, &d_len, &d_status, true, &stats.launches)) != MD_OK) return rc;
    HIP_TRY(ctx, md::to_host(dl_len.data(), d_len, np, st));
    HIP_TRY(ctx, md::to_host(dl_status.data(), d_status, np, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    stats.score_ns = pkw_event_ns(ctx);
    for (size_t k = 0; k < np; k++) stats.fitted += fitted[k] = dl_status[k] == MD_OK;
  }

  // -- the choice
  t0 = std::chrono::steady_clock::now();
  std::vector<uint64_t> base(n);
  std::vector<uint32_t> depth(n);
  stats.chosen = md::pks::choose(n, cand, dl_len.data(), fitted.data(), max_depth, base.data(), depth.data());
  for (size_t r = 0; r < n; r++) {
    const md_pack_source &o = objs[order[r]];
    sorted[r].off = o.off, sorted[r].len = o.len, sorted[r].base = base[r], sorted[r].type = o.type;
  }
  stats.host_ns += ns_since(t0);
  return MD_OK;
}

}  // namespace

int md_pack_choose_bases(md_ctx *ctx, uint32_t window, uint32_t max_depth, size_t n, const md_pack_source *objs, const uint8_t *src, size_t src_len,
                         md_pack_source *sorted, uint64_t *order) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  ctx->pack_search_last = {};
  if (window < 1 || window > md::pks::kMaxWindow) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_choose_bases: window is 1 .. 64");
  if (n > md::pks::kMaxPairs / (md::pks::kFeatures * window)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_choose_bases: too many objects for this window");
  if (n == 0) return MD_OK;
  if (!objs || !sorted || !order || (!src && src_len)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_choose_bases: null pointer");
  for (size_t i = 0; i < n; i++) {
    const md_pack_source &o = objs[i];
    if (o.type < 1 || o.type > 4) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_choose_bases: a type is 1 .. 4");
    if (o.len > MD_MAX_STREAM || o.off > src_len || o.len > src_len - o.off) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_choose_bases: an object beyond the source, or too long");
  }
  const int rc = no_bad_alloc(ctx, "host memory for the search", [&] { return choose_bases(ctx, window, max_depth, n, objs, src, src_len, sorted, order); });
  // (the events are the delta batch's: what md_pack_write_last would read from them is this call's)
  ctx->pack_write_last = {};
  ctx->pack_write_last.pairs = ctx->pack_search_last.pairs, ctx->pack_write_last.delta_ns = ctx->pack_search_last.score_ns;
  ctx->pkw_pending = false;
  return rc;
}

int md_pack_search_last(const md_ctx *ctx, md_pack_search_stats *stats) {
  if (!ctx || !stats) return MD_E_INVALID_ARGUMENT;
  *stats = ctx->pack_search_last;
  return MD_OK;
}
