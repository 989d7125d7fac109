// capi_pack_graph.cpp — the object graph of a git pack (mdeflate.h: md_pack_graph_build, md_pack_graph_get, md_pack_graph_edges,
// md_pack_graph_status, md_pack_reachable, md_pack_reach_last, md_pack_graph_free).  The build is md_pack_verify's plan and
// rounds (pack_link_rounds, capi_pack.cpp) over every sound commit, tree and tag, with the link kernels behind each round's
// last apply launch (pack_graph_kernels.hip; the parse rules are pack_graph.hpp's); the edges leave their bound-sized slots
// by one scan and one gather.  A walk closes the roots over parents and tag targets on the host and follows all edges on
// the device, one launch a frontier.
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "pack_graph.hpp"

namespace {
namespace pg = md::pg;

int graph_build(md_ctx *ctx, const md_pack *P, const uint8_t *pack, unsigned flags, md_pack_graph *G) {
  const size_t n = P->objs.size();
  G->device = ctx->device;
  memcpy(G->pack_checksum, P->pack_checksum, 20);
  G->info.n = n;
  G->first.assign(n + 1, 0);
  G->hist_first.assign(n + 1, 0);
  G->status.resize(n);
  for (size_t i = 0; i < n; i++) G->status[i] = P->objs[i].status;
  if (n == 0) return MD_OK;

  // -- what is decoded, and where every object's edges go until their number is known
  std::vector<uint64_t> select, slot_off(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    const md_pack_object &o = P->objs[i];
    const bool mine = o.status == MD_OK && (o.type == 1 || o.type == 2 || o.type == 4);
    if (mine) select.push_back(i);
    slot_off[i + 1] = slot_off[i] + (mine ? pg::edge_bound(o.type, o.size) : 0);
  }
  const uint64_t slots = slot_off[n];
  std::vector<uint8_t> names(n * 20), type(n);
  for (size_t i = 0; i < n; i++) memcpy(&names[i * 20], P->objs[i].name, 20), type[i] = (uint8_t)P->objs[i].type;

  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  PackLinkSink sink;
  md::pkg::Links &l = sink.links;
  uint8_t *d_names = nullptr, *d_type = nullptr;
  uint32_t *d_fan = nullptr;
  uint64_t *d_slot_off = nullptr, *d_first = nullptr;
  int rc = carve(ctx, ctx->scratch[kPkgDesc], "hipMalloc(pack graph tables)", [&](md::Carver &c) {
    d_names = c.take<uint8_t>(n * 20), d_fan = c.take<uint32_t>(256), d_type = c.take<uint8_t>(n);
    d_slot_off = c.take<uint64_t>(n + 1), d_first = c.take<uint64_t>(n + 1);
    l.deg = c.take<uint32_t>(n), l.bad = c.take<uint8_t>(n);
  });
  if (rc == MD_OK)
    rc = carve(ctx, ctx->scratch[kPkgSlots], "hipMalloc(pack graph edge slots)", [&](md::Carver &c) { l.to = c.take<uint32_t>(slots), l.kind = c.take<uint8_t>(slots); });
  if (rc != MD_OK) return rc;
  l.names = d_names, l.fan = d_fan, l.type = d_type, l.n = n, l.slot_off = d_slot_off;
  HIP_TRY(ctx, md::to_device(d_names, names, st));
  HIP_TRY(ctx, md::to_device(d_fan, P->fan, 256, st));
  HIP_TRY(ctx, md::to_device(d_type, type, st));
  HIP_TRY(ctx, md::to_device(d_slot_off, slot_off, st));
  HIP_TRY(ctx, md::zero(l.deg, n, st));
  HIP_TRY(ctx, md::zero(l.bad, n, st));

  // -- the rounds (they wait for the stream)
  std::vector<int32_t> status(select.size());
  md_pack_result res = {};
  if ((rc = pack_link_rounds(ctx, P, pack, select.data(), select.size(), flags, status.data(), &res, &sink)) != MD_OK) return rc;
  G->info.parsed = ctx->pack_last.objects;
  G->info.rounds = ctx->pack_last.rounds;
  G->info.parse_launches = sink.launches;
  G->info.device_ns = sink.device_ns;

  // -- the counts scanned, the edges out of their slots in idx order
  std::vector<uint8_t> bad(n);
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan32(l.deg, n, d_first, st));
  HIP_TRY(ctx, md::to_host(G->first.data(), d_first, n + 1, st));
  HIP_TRY(ctx, md::to_host(bad.data(), l.bad, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  const uint64_t edges = G->first[n];
  if ((rc = G->d_first.reserve(ctx, (n + 1) * sizeof(uint64_t), "hipMalloc(pack graph)")) != MD_OK) return rc;
  if ((rc = G->d_to.reserve(ctx, edges * sizeof(uint32_t), "hipMalloc(pack graph)")) != MD_OK) return rc;
  if ((rc = G->d_kind.reserve(ctx, edges, "hipMalloc(pack graph)")) != MD_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(G->d_first.p, d_first, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  MD_LAUNCH_TRY(ctx, md_launch_pkg_gather(n, edges, d_slot_off, d_first, l.to, l.kind, G->d_to.as<uint32_t>(), G->d_kind.as<uint8_t>(), st));
  std::vector<uint32_t> to(edges);
  std::vector<uint8_t> kind(edges);
  HIP_TRY(ctx, md::to_host(to.data(), G->d_to.as<uint32_t>(), edges, st));
  HIP_TRY(ctx, md::to_host(kind.data(), G->d_kind.as<uint8_t>(), edges, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));

  // -- the host's part: statuses, counts, the edges of the history
  for (size_t j = 0; j < select.size(); j++) {
    const size_t i = (size_t)select[j];
    G->status[i] = status[j] == MD_OK && bad[i] ? MD_INVALID_OBJECT : status[j];
  }
  for (size_t i = 0; i < n; i++) {
    G->info.malformed += G->status[i] == MD_INVALID_OBJECT;
    G->info.failed += G->status[i] != MD_OK && G->status[i] != MD_INVALID_OBJECT;
    for (uint64_t e = G->first[i]; e < G->first[i + 1]; e++) {
      const uint32_t k = kind[e] & 0x3f;
      G->info.absent += (kind[e] & pg::kAbsent) != 0;
      G->info.mistyped += (kind[e] & pg::kMistyped) != 0;
      if ((k == pg::kCommitParent || k == pg::kTagTarget) && to[e] != pg::kNoLink) G->hist_to.push_back(to[e]);
    }
    G->hist_first[i + 1] = G->hist_to.size();
  }
  G->info.edges = edges;
  return MD_OK;
}

// One walk: marks (n words, zeroed here) = the roots and what is reached from them.  The host closes the roots over the
// history's edges; what it reached is marked and, where it has edges, stands on the first frontier.
struct Walk {
  uint32_t *mark, *seed, *front[2], *next_len;
};
int walk(md_ctx *ctx, const md_pack_graph *G, const uint64_t *roots, size_t nroots, const Walk &w, md::PairTimers *timers, md_pack_reach_stats *stats) {
  const size_t n = G->first.size() - 1;
  hipStream_t st = ctx->stream;
  std::vector<uint8_t> seen(n, 0);
  std::vector<uint32_t> closed, frontier;
  for (size_t k = 0; k < nroots; k++)
    if (!seen[roots[k]]) seen[roots[k]] = 1, closed.push_back((uint32_t)roots[k]);
  for (size_t k = 0; k < closed.size(); k++)  // (it grows as it is walked)
    for (uint64_t e = G->hist_first[closed[k]]; e < G->hist_first[closed[k] + 1]; e++)
      if (!seen[G->hist_to[e]]) seen[G->hist_to[e]] = 1, closed.push_back(G->hist_to[e]);
  for (uint32_t o : closed)
    if (G->first[o] != G->first[o + 1]) frontier.push_back(o);
  stats->host_closed += closed.size();
  stats->seeds += frontier.size();
  HIP_TRY(ctx, md::zero(w.mark, n, st));
  HIP_TRY(ctx, md::to_device(w.seed, closed, st));
  HIP_TRY(ctx, md::to_device(w.front[0], frontier, st));
  MD_LAUNCH_TRY(ctx, md_launch_pkg_seed((uint32_t)closed.size(), w.seed, w.mark, st));
  md::pkg::Reach r = {G->d_first.as<uint64_t>(), G->d_to.as<uint32_t>(), w.mark, nullptr, w.next_len};
  uint32_t len = (uint32_t)frontier.size();
  for (int cur = 0; len != 0; cur ^= 1) {  // one launch per non-empty frontier; the next one's length comes back
    r.next = w.front[cur ^ 1];
    HIP_TRY(ctx, md::zero(w.next_len, 1, st));
    timers->mark(st);
    MD_LAUNCH_TRY(ctx, md_launch_pkg_reach_step(&r, w.front[cur], len, st));
    timers->mark(st);
    stats->rounds++;
    stats->expanded += len;
    HIP_TRY(ctx, md::to_host(&len, w.next_len, 1, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (closed and frontier were copied from)
  return MD_OK;
}

int reachable(md_ctx *ctx, const md_pack_graph *G, const uint64_t *roots, size_t nroots, const uint64_t *exclude, size_t nexclude, uint8_t *mark,
              uint64_t *count) {
  const size_t n = G->first.size() - 1;
  md_pack_reach_stats &stats = ctx->pack_reach_last;
  stats = {};
  *count = 0;
  if (n == 0) return MD_OK;
  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  Walk w = {}, x = {};
  uint8_t *d_out = nullptr;
  uint32_t *d_count = nullptr;
  int rc = carve(ctx, ctx->scratch[kPkgDesc], "hipMalloc(pack graph walk)", [&](md::Carver &c) {
    w.mark = c.take<uint32_t>(n), x.mark = c.take<uint32_t>(nexclude ? n : 0);
    w.seed = x.seed = c.take<uint32_t>(n);
    w.front[0] = x.front[0] = c.take<uint32_t>(n), w.front[1] = x.front[1] = c.take<uint32_t>(n);
    w.next_len = x.next_len = c.take<uint32_t>(1);
    d_count = c.take<uint32_t>(1), d_out = c.take<uint8_t>(n);
  });
  if (rc != MD_OK) return rc;
  md::PairTimers timers;
  if (nexclude && (rc = walk(ctx, G, exclude, nexclude, x, &timers, &stats)) != MD_OK) return rc;
  if ((rc = walk(ctx, G, roots, nroots, w, &timers, &stats)) != MD_OK) return rc;
  uint32_t marked = 0;
  HIP_TRY(ctx, md::zero(d_count, 1, st));
  timers.mark(st);
  MD_LAUNCH_TRY(ctx, md_launch_pkg_reach_finish(n, w.mark, nexclude ? x.mark : nullptr, d_out, d_count, st));
  timers.mark(st);
  HIP_TRY(ctx, md::to_host(mark, d_out, n, st));
  HIP_TRY(ctx, md::to_host(&marked, d_count, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  stats.marked = *count = marked;
  stats.device_ns = timers.total_ns();
  return MD_OK;
}
}  // namespace

int md_pack_graph_build(md_ctx *ctx, const md_pack *p, const uint8_t *pack, size_t pack_len, unsigned flags, md_pack_graph **g) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!g) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  *g = nullptr;
  if (!p || !pack) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  if (flags & ~MD_PACK_VERIFY_CRC) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_graph_build: unknown flag");
  if (pack_len != p->pack_len || memcmp(pack + pack_len - 20, p->pack_checksum, 20) != 0)
    return fail(ctx, MD_INVALID_INDEX, "md_pack_graph_build: the table belongs to another pack");
  md_pack_graph *G = new (std::nothrow) md_pack_graph();
  if (!G) return fail(ctx, MD_E_OUT_OF_MEMORY, "host memory for the pack's graph");
  const int rc = no_bad_alloc(ctx, "host memory for the pack's graph", [&] { return graph_build(ctx, p, pack, flags, G); });
  if (rc != MD_OK) {
    md_pack_graph_free(G);
    return rc;
  }
  *g = G;
  return MD_OK;
}

int md_pack_graph_get(const md_pack_graph *g, md_pack_graph_info *info) {
  if (!g || !info) return MD_E_INVALID_ARGUMENT;
  *info = g->info;
  return MD_OK;
}

int md_pack_graph_edges(const md_pack_graph *g, uint64_t *first, uint32_t *to, uint8_t *kind, size_t cap) {
  if (!g) return MD_E_INVALID_ARGUMENT;
  if (cap == 0 && !first && !to && !kind) return MD_OK;  // the size query: md_pack_graph_get's edges
  if (!first || ((!to || !kind) && g->info.edges)) return MD_E_INVALID_ARGUMENT;
  if (cap < g->info.edges) return MD_UNEXPECTED_END_OF_OUTPUT;
  memcpy(first, g->first.data(), g->first.size() * sizeof(uint64_t));
  if (g->info.edges == 0) return MD_OK;
  md::DeviceGuard guard(g->device);
  if (!guard.ok) return MD_E_HIP;
  if (hipMemcpy(to, g->d_to.p, (size_t)g->info.edges * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(kind, g->d_kind.p, (size_t)g->info.edges, hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    return MD_E_HIP;
  }
  return MD_OK;
}

int md_pack_graph_status(const md_pack_graph *g, int32_t *status) {
  if (!g || (!status && !g->status.empty())) return MD_E_INVALID_ARGUMENT;
  if (!g->status.empty()) memcpy(status, g->status.data(), g->status.size() * sizeof(int32_t));
  return MD_OK;
}

int md_pack_reachable(md_ctx *ctx, const md_pack_graph *g, const uint64_t *roots, size_t nroots, const uint64_t *exclude, size_t nexclude,
                      uint8_t *mark, uint64_t *count) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!g || !count || (nroots && !roots) || (nexclude && !exclude)) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  const size_t n = g->first.size() - 1;
  if (n && !mark) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  if (g->device != ctx->device) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_reachable: the graph lives on another device");
  for (size_t k = 0; k < nroots; k++)
    if (roots[k] >= n) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_reachable: root out of range");
  for (size_t k = 0; k < nexclude; k++)
    if (exclude[k] >= n) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_reachable: excluded object out of range");
  return no_bad_alloc(ctx, "host memory for the walk", [&] { return reachable(ctx, g, roots, nroots, exclude, nexclude, mark, count); });
}

int md_pack_reach_last(const md_ctx *ctx, md_pack_reach_stats *stats) {
  if (!ctx || !stats) return MD_E_INVALID_ARGUMENT;
  *stats = ctx->pack_reach_last;
  return MD_OK;
}

void md_pack_graph_free(md_pack_graph *g) {
  if (!g) return;
  md::DeviceGuard guard(g->device);  // (the buffers are freed on their device; hipFree waits for what still uses them)
  delete g;
}
