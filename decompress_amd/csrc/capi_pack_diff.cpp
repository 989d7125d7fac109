// capi_pack_diff.cpp — trees of a git pack diffed (mdeflate.h: md_pack_diff, md_pack_diff_get, md_pack_diff_changes,
// md_pack_diff_status, md_pack_diff_free).  The recursion advances a level a time over all pairs at once: the host lists the
// level's distinct trees, the read decodes them and leaves them on the device (pack_read_resident, capi_pack.cpp), the table
// kernel writes every tree's entries once, the diff kernel counts, two scans place the records, the diff kernel writes them
// (pack_diff_kernels.hip; the rules are pack_diff.hpp's), and the host derives the next level's sub-pairs from the records.
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "pack_diff.hpp"

struct md_pack_diff_result {
  md_pack_diff_info info = {};
  std::vector<md_tree_change> changes;
  std::vector<uint8_t> names;
  std::vector<int32_t> status;
};

namespace {
namespace pd = md::pd;
namespace pkd = md::pkd;

// a pair of a level: objects of the table or pd::kNone, the caller's pair, the directory record it came from
struct LevelPair {
  uint32_t a, b, id, parent;
};

int diff_run(md_ctx *ctx, const md_pack *P, const md_pack_graph *G, const uint8_t *pack, size_t npairs, const uint32_t *a, const uint32_t *b,
             bool recursive, md_pack_diff_result *R) {
  md_pack_diff_info &info = R->info;
  info.pairs = npairs;
  R->status.assign(npairs, MD_OK);
  // a tree the diff can ask the read for; what it says of one it cannot
  const auto eligible = [&](uint32_t o) { return G->status[o] == MD_OK && P->objs[o].type == 2; };
  const auto refusal = [&](uint32_t o) { return G->status[o] != MD_OK ? G->status[o] : (int32_t)MD_INVALID_OBJECT; };
  std::vector<LevelPair> level, next;
  for (size_t q = 0; q < npairs; q++) {
    if (a[q] == b[q]) continue;
    if (a[q] != pd::kNone && !eligible(a[q])) R->status[q] = refusal(a[q]);
    else if (b[q] != pd::kNone && !eligible(b[q])) R->status[q] = refusal(b[q]);
    else level.push_back(LevelPair{a[q], b[q], (uint32_t)q, pd::kNone});
  }

  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  md::PairTimers timers;
  bool uploaded = false;
  while (!level.empty()) {
    // -- the level's distinct trees, ascending, and every pair's sides among them
    std::vector<uint64_t> trees;
    for (const LevelPair &l : level) {
      if (l.a != pd::kNone) trees.push_back(l.a);
      if (l.b != pd::kNone) trees.push_back(l.b);
    }
    std::sort(trees.begin(), trees.end());
    trees.erase(std::unique(trees.begin(), trees.end()), trees.end());
    const size_t T = trees.size(), np = level.size();
    if (T > 0x7ffffff0ull || np > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_diff: too many pairs in one level");
    const auto slot_of = [&](uint32_t o) { return o == pd::kNone ? pd::kNone : (uint32_t)(std::lower_bound(trees.begin(), trees.end(), (uint64_t)o) - trees.begin()); };
    std::vector<uint32_t> pa(np), pb(np), pid(np), pparent(np);
    for (size_t q = 0; q < np; q++) pa[q] = slot_of(level[q].a), pb[q] = slot_of(level[q].b), pid[q] = level[q].id, pparent[q] = level[q].parent;

    // -- decoded, and kept where the rounds put them
    std::vector<uint64_t> off(T + 1), size(T), row_off(T + 1, 0);
    std::vector<int32_t> rstatus(T);
    std::vector<uint32_t> obj(T);
    md_pack_result res = {};
    const uint8_t *d_buf = nullptr;
    int rc = pack_read_resident(ctx, P, uploaded ? nullptr : pack, trees.data(), T, off.data(), rstatus.data(), &res, &d_buf);
    if (rc != MD_OK) return rc;
    uploaded = true;
    info.trees_read += T;
    info.levels++;
    for (size_t t = 0; t < T; t++) {
      obj[t] = (uint32_t)trees[t], size[t] = P->objs[trees[t]].size;
      row_off[t + 1] = row_off[t] + size[t] / md::pg::kMinEntry;
    }

    // -- tables, counts, places
    pkd::Trees dt = {};
    pkd::Pairs dp = {};
    uint64_t *d_off = nullptr, *d_size = nullptr, *d_row_off = nullptr, *d_rec_first = nullptr, *d_name_first = nullptr;
    int32_t *d_status = nullptr;
    uint32_t *d_obj = nullptr, *d_a = nullptr, *d_b = nullptr, *d_id = nullptr, *d_parent = nullptr;
    rc = carve(ctx, ctx->scratch[kPkdDesc], "hipMalloc(pack diff tables)", [&](md::Carver &c) {
      d_off = c.take<uint64_t>(T), d_size = c.take<uint64_t>(T), d_row_off = c.take<uint64_t>(T);
      d_status = c.take<int32_t>(T), d_obj = c.take<uint32_t>(T);
      dt.rows = c.take<pkd::Row>(row_off[T]), dt.cnt = c.take<uint32_t>(T), dt.ok = c.take<uint8_t>(T);
      d_a = c.take<uint32_t>(np), d_b = c.take<uint32_t>(np), d_id = c.take<uint32_t>(np), d_parent = c.take<uint32_t>(np);
      dp.nrec = c.take<uint32_t>(np), dp.nbytes = c.take<uint64_t>(np);
      d_rec_first = c.take<uint64_t>(np + 1), d_name_first = c.take<uint64_t>(np + 1);
    });
    if (rc != MD_OK) return rc;
    dt.count = (uint32_t)T, dt.off = d_off, dt.size = d_size, dt.row_off = d_row_off, dt.status = d_status, dt.obj = d_obj;
    dp.count = (uint32_t)np, dp.a = d_a, dp.b = d_b, dp.id = d_id, dp.parent = d_parent;
    dp.first = G->d_first.as<uint64_t>(), dp.to = G->d_to.as<uint32_t>();
    dp.rec_first = d_rec_first, dp.name_first = d_name_first, dp.name_base = R->names.size();
    HIP_TRY(ctx, md::to_device(d_off, off.data(), T, st));
    HIP_TRY(ctx, md::to_device(d_size, size, st));
    HIP_TRY(ctx, md::to_device(d_row_off, row_off.data(), T, st));
    HIP_TRY(ctx, md::to_device(d_status, rstatus, st));
    HIP_TRY(ctx, md::to_device(d_obj, obj, st));
    HIP_TRY(ctx, md::to_device(d_a, pa, st));
    HIP_TRY(ctx, md::to_device(d_b, pb, st));
    HIP_TRY(ctx, md::to_device(d_id, pid, st));
    HIP_TRY(ctx, md::to_device(d_parent, pparent, st));
    timers.mark(st);
    MD_LAUNCH_TRY(ctx, md_launch_pkd_tree_table(&dt, d_buf, st));
    MD_LAUNCH_TRY(ctx, md_launch_pkd_tree_diff(&dt, &dp, d_buf, 0, st));
    timers.mark(st);
    MD_LAUNCH_TRY(ctx, md_launch_gzm_scan32(dp.nrec, np, d_rec_first, st));
    MD_LAUNCH_TRY(ctx, md_launch_gzm_scan64(dp.nbytes, np, d_name_first, st));
    info.launches += 4;
    uint64_t nrec = 0, nbytes = 0;
    std::vector<uint8_t> ok(T);
    HIP_TRY(ctx, md::to_host(&nrec, d_rec_first + np, 1, st));
    HIP_TRY(ctx, md::to_host(&nbytes, d_name_first + np, 1, st));
    HIP_TRY(ctx, md::to_host(ok.data(), dt.ok, T, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));

    // -- the records and their names
    const size_t rec_base = R->changes.size(), name_base = R->names.size();
    if (rec_base + nrec > 0xfffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_diff: too many records");
    if (nrec != 0) {
      rc = carve(ctx, ctx->scratch[kPkdOut], "hipMalloc(pack diff records)",
                 [&](md::Carver &c) { dp.out = c.take<md_tree_change>(nrec), dp.names = c.take<uint8_t>(nbytes); });
      if (rc != MD_OK) return rc;
      timers.mark(st);
      MD_LAUNCH_TRY(ctx, md_launch_pkd_tree_diff(&dt, &dp, d_buf, 1, st));
      timers.mark(st);
      info.launches++;
      R->changes.resize(rec_base + nrec);
      R->names.resize(name_base + nbytes);
      HIP_TRY(ctx, md::to_host(R->changes.data() + rec_base, dp.out, nrec, st));
      HIP_TRY(ctx, md::to_host(R->names.data() + name_base, dp.names, nbytes, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
    }

    // -- the host's part: what a side that turned out unreadable means, and the next level's pairs
    for (size_t q = 0; q < np; q++) {
      const uint32_t bad = pa[q] != pd::kNone && !ok[pa[q]] ? pa[q] : pb[q] != pd::kNone && !ok[pb[q]] ? pb[q] : pd::kNone;
      if (bad == pd::kNone) continue;
      if (level[q].parent == pd::kNone) R->status[level[q].id] = rstatus[bad] != MD_OK ? rstatus[bad] : (int32_t)MD_INVALID_OBJECT;
      else R->changes[level[q].parent].flags |= MD_TREE_CHANGE_OPAQUE;
    }
    next.clear();
    for (size_t r = rec_base; recursive && r < R->changes.size(); r++) {
      md_tree_change &c = R->changes[r];
      if (!(c.flags & MD_TREE_CHANGE_TREE)) continue;
      const bool in_a = c.kind != 'A', in_b = c.kind != 'D';
      if ((in_a && (c.a_obj == MD_PACK_NO_LINK || !eligible(c.a_obj))) || (in_b && (c.b_obj == MD_PACK_NO_LINK || !eligible(c.b_obj)))) {
        c.flags |= MD_TREE_CHANGE_OPAQUE;
        continue;
      }
      if (in_a && in_b && c.a_obj == c.b_obj) continue;  // (two names of one object: forged)
      next.push_back(LevelPair{in_a ? c.a_obj : pd::kNone, in_b ? c.b_obj : pd::kNone, c.pair, (uint32_t)r});
    }
    level.swap(next);
  }
  info.device_ns = timers.total_ns();
  info.changes = R->changes.size();
  info.name_bytes = R->names.size();
  for (const md_tree_change &c : R->changes) info.opaque += (c.flags & MD_TREE_CHANGE_OPAQUE) != 0;
  for (int32_t s : R->status) info.failed += s != MD_OK;
  return MD_OK;
}
}  // namespace

int md_pack_diff(md_ctx *ctx, const md_pack *p, const md_pack_graph *g, const uint8_t *pack, size_t pack_len, size_t npairs, const uint32_t *a,
                 const uint32_t *b, unsigned flags, md_pack_diff_result **r) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!r) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  *r = nullptr;
  if (!p || !g || !pack || (npairs && (!a || !b))) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  if (flags & ~MD_PACK_DIFF_RECURSIVE) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_diff: unknown flag");
  if (pack_len != p->pack_len || memcmp(pack + pack_len - 20, p->pack_checksum, 20) != 0)
    return fail(ctx, MD_INVALID_INDEX, "md_pack_diff: the table belongs to another pack");
  const size_t n = p->objs.size();
  if (g->first.size() != n + 1 || memcmp(g->pack_checksum, p->pack_checksum, 20) != 0)
    return fail(ctx, MD_INVALID_INDEX, "md_pack_diff: the graph belongs to another table");
  if (g->device != ctx->device) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_diff: the graph lives on another device");
  if (npairs > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_diff: too many pairs");
  for (size_t q = 0; q < npairs; q++)
    if ((a[q] != MD_TREE_NONE && a[q] >= n) || (b[q] != MD_TREE_NONE && b[q] >= n)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_diff: tree out of range");
  md_pack_diff_result *R = new (std::nothrow) md_pack_diff_result();
  if (!R) return fail(ctx, MD_E_OUT_OF_MEMORY, "host memory for the diff");
  const int rc = no_bad_alloc(ctx, "host memory for the diff", [&] { return diff_run(ctx, p, g, pack, npairs, a, b, (flags & MD_PACK_DIFF_RECURSIVE) != 0, R); });
  if (rc != MD_OK) {
    delete R;
    return rc;
  }
  *r = R;
  return MD_OK;
}

int md_pack_diff_get(const md_pack_diff_result *r, md_pack_diff_info *info) {
  if (!r || !info) return MD_E_INVALID_ARGUMENT;
  *info = r->info;
  return MD_OK;
}

int md_pack_diff_changes(const md_pack_diff_result *r, md_tree_change *changes, size_t cap, uint8_t *names, size_t names_cap) {
  if (!r) return MD_E_INVALID_ARGUMENT;
  if (cap == 0 && names_cap == 0 && !changes && !names) return MD_OK;  // the size query: md_pack_diff_get's changes and name_bytes
  if ((!changes && !r->changes.empty()) || (!names && !r->names.empty())) return MD_E_INVALID_ARGUMENT;
  if (cap < r->changes.size() || names_cap < r->names.size()) return MD_UNEXPECTED_END_OF_OUTPUT;
  if (!r->changes.empty()) memcpy(changes, r->changes.data(), r->changes.size() * sizeof(md_tree_change));
  if (!r->names.empty()) memcpy(names, r->names.data(), r->names.size());
  return MD_OK;
}

int md_pack_diff_status(const md_pack_diff_result *r, int32_t *status) {
  if (!r || (!status && !r->status.empty())) return MD_E_INVALID_ARGUMENT;
  if (!r->status.empty()) memcpy(status, r->status.data(), r->status.size() * sizeof(int32_t));
  return MD_OK;
}

void md_pack_diff_free(md_pack_diff_result *r) { delete r; }
