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

// features preset to all ones and the sketch launch, on the context's stream, with `span` (or none: null) around the launch
// alone.  d_features null: they are carved from kPkwDesc behind the segments (*features says where).  Nothing is read back.
int enqueue_sketch(md_ctx *ctx, size_t n, const std::vector<md::pks::Seg> &segs, const uint8_t *d_src, uint32_t *d_features, uint32_t **features,
                   md::EventSpan *span, uint64_t *launches) {
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
  if (span) HIP_TRY(ctx, span->begin(st));
  if (!segs.empty()) {
    MD_LAUNCH_TRY(ctx, md_launch_pks_sketch((uint32_t)segs.size(), d_segs, d_src, *features, st));
    ++*launches;
  }
  if (span) HIP_TRY(ctx, span->end(st));
  return MD_OK;
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
    return enqueue_sketch(ctx, n, segs, d_src, d_features, &features, nullptr, &launches);
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
    return enqueue_sketch(ctx, n, segs, ctx->scratch[kHostIn].as<uint8_t>(), nullptr, &d_features, nullptr, &launches);
  });
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_host(features, d_features, n * md::pks::kFeatures, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MD_OK;
}

int md_pack_delta_sizes_device(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *d_src, uint64_t *d_out_len, int32_t *d_status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n && (!pairs || !d_src || !d_out_len || !d_status)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_delta_sizes_device: null pointer");
  return delta_batch(ctx, false, DeltaKind::kSizes, n, pairs, d_src, 0, nullptr, 0, DeltaResults{d_out_len, d_status});
}

int md_pack_delta_sizes_host(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *src, size_t src_len, uint64_t *out_len,
                             int32_t *status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n && (!pairs || (!src && src_len) || !out_len || !status)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_delta_sizes_host: null pointer");
  return delta_batch(ctx, true, DeltaKind::kSizes, n, pairs, src, src_len, nullptr, 0, DeltaResults{out_len, status});
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
  if ((rc = enqueue_sketch(ctx, n, segs, d_src, nullptr, &d_features, &ctx->pkw_span, &stats.launches)) != MD_OK) return rc;
  std::vector<uint32_t> features(n * md::pks::kFeatures);
  HIP_TRY(ctx, md::to_host(features.data(), d_features, features.size(), st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  stats.sketch_ns = ctx->pkw_span.ns();

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
  std::vector<uint8_t> is_base(n, 0);
  for (size_t k = 0; k < np; k++) is_base[cand.base[k]] = 1;
  std::vector<md::pkw::TablePlace> place(n);
  for (size_t r = 0; r < n; r++)
    if (is_base[r]) place[r] = plan.add_base(objs[order[r]].off, objs[order[r]].len);  // (a block at least: a candidate has features)
  for (size_t t = 0; t < n; t++) {
    const md_pack_source &o = objs[order[t]];
    for (uint64_t k = cand.first[t]; k < cand.first[t + 1]; k++) {
      const md_pack_source &b = objs[order[cand.base[k]]];
      plan.pairs[k] = DeltaPlan::pair(md_pack_delta_pair{b.off, b.len, o.off, o.len, 0, md::pkw::delta_cap(o.len)}, place[cand.base[k]]);
    }
  }
  stats.host_ns = ns_since(t0);

  // -- scores: one index launch over the distinct candidates, one size launch over the pairs
  std::vector<uint64_t> dl_len(np);
  std::vector<int32_t> dl_status(np);
  std::vector<uint8_t> fitted(np);
  if (np) {
    DeltaResults d;
    if ((rc = enqueue_delta_plan(ctx, plan, d_src, DeltaKind::kSizes, nullptr, &d, &stats.launches)) != MD_OK) return rc;
    HIP_TRY(ctx, md::to_host(dl_len.data(), d.out_len, np, st));
    HIP_TRY(ctx, md::to_host(dl_status.data(), d.status, np, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    stats.score_ns = ctx->pkw_span.ns();
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
  int rc = check_sources(ctx, "md_pack_choose_bases", n, objs, src_len);
  if (rc != MD_OK) return rc;
  rc = no_bad_alloc(ctx, "host memory for the search", [&] { return choose_bases(ctx, window, max_depth, n, objs, src, src_len, sorted, order); });
  // (the span is the delta batch's: what md_pack_write_last would read from it is this call's)
  ctx->pack_write_last = {};
  ctx->pack_write_last.pairs = ctx->pack_search_last.pairs, ctx->pack_write_last.delta_ns = ctx->pack_search_last.score_ns;
  ctx->pkw_span.pending = false;
  return rc;
}

int md_pack_search_last(const md_ctx *ctx, md_pack_search_stats *stats) {
  if (!ctx || !stats) return MD_E_INVALID_ARGUMENT;
  *stats = ctx->pack_search_last;
  return MD_OK;
}
