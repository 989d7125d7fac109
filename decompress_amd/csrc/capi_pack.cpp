// capi_pack.cpp — git packfiles (mdeflate.h: md_pack_index, md_pack_open, md_pack_get, md_pack_objects, md_pack_find,
// md_pack_free, md_pack_read, md_pack_verify, md_pack_last).  The idx is the host's (pack_index.hpp), and so are the sort
// of its offsets, the plan of a read and the last walk over the table in order of depth; headers, chains, sizes, statuses
// and the deltas' instructions are the device's (pack_kernels.hip), the zlib streams the batch decoder's, the names'
// SHA-1s capi_sha1.cpp's (sha1_enqueue).  The table builder behind the idx (pack_table) and the rounds of a verification
// with a hash pass that writes names (pack_verify_names) are also md_pack_index_build's (capi_pack_build.cpp; ctx.hpp).
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "pack_index.hpp"

namespace {
using md::pk::Delta;
using md::pk::Repeat;
using md::pk::Stream;

constexpr uint32_t kNone = 0xffffffffu;
// a slot of scratch: the bytes and room for the copy loops' 16-byte reads, on 64 bytes
inline uint64_t slot_stride(uint64_t cap) { return ((cap + 63) & ~(uint64_t)63) + 64; }

// the inflate launch's descriptors of `count` streams and what comes behind it, carved from one block
struct RoundDesc {
  Stream *rows = nullptr;
  uint64_t *in_off = nullptr, *in_len = nullptr, *out_off = nullptr, *out_cap = nullptr, *out_len = nullptr, *consumed = nullptr, *p_off = nullptr,
           *p_len = nullptr, *base_size = nullptr, *result_size = nullptr;
  uint32_t *crc = nullptr;
  int32_t *status = nullptr;
  Delta *deltas = nullptr;
  Repeat *repeats = nullptr;
  // the link pass of md_pack_graph_build (nlink = count, else 0): where every stream's object stands, its size, type and
  // object, and the streams that are trees / commits and tags
  uint64_t *l_off = nullptr, *l_size = nullptr;
  uint32_t *l_obj = nullptr, *l_trees = nullptr, *l_others = nullptr;
  uint8_t *l_type = nullptr;
  void carve(md::Carver *c, size_t count, size_t ndelta, size_t nrepeat, size_t nlink = 0) {
    rows = c->take<Stream>(count);
    uint64_t **m64[10] = {&in_off, &in_len, &out_off, &out_cap, &out_len, &consumed, &p_off, &p_len, &base_size, &result_size};
    for (uint64_t **p : m64) *p = c->take<uint64_t>(count);
    crc = c->take<uint32_t>(count);
    status = c->take<int32_t>(count);
    deltas = c->take<Delta>(ndelta);
    repeats = c->take<Repeat>(nrepeat);
    l_off = c->take<uint64_t>(nlink), l_size = c->take<uint64_t>(nlink);
    l_obj = c->take<uint32_t>(nlink), l_trees = c->take<uint32_t>(nlink), l_others = c->take<uint32_t>(nlink);
    l_type = c->take<uint8_t>(nlink);
  }
};

// the host side of a round's streams: the rows, the inflate launch's descriptors and the CRC launch's (p_off and p_len:
// inflate_round reads them with `verify` alone, so md_pack_open's rounds fill them for nothing)
struct RoundStreams {
  std::vector<Stream> rows;
  std::vector<uint64_t> in_off, in_len, out_off, out_cap, p_off, p_len;
  // the object at pack[off, off + packed) whose zlib stream begins at zoff and inflates to hsize bytes at `out`
  void add(uint64_t off, uint64_t packed, uint64_t zoff, uint64_t hsize, uint32_t crc, uint64_t out) {
    const uint64_t zlen = off + packed - zoff;
    rows.push_back(Stream{off, packed, zlen, hsize, crc, 0});
    in_off.push_back(zoff), in_len.push_back(zlen), out_off.push_back(out), out_cap.push_back(hsize);
    p_off.push_back(off), p_len.push_back(packed);
  }
};

// The streams of h (it lives until the stream has been waited for) of the pack at d_pack, stream j into d_buf + h.out_off[j]:
// one inflate launch, the CRC-32s of the packed bytes if asked for, and the verdicts (left in d.status).
int inflate_round(md_ctx *ctx, const RoundDesc &d, const uint8_t *d_pack, uint8_t *d_buf, const RoundStreams &h, bool verify) {
  hipStream_t st = ctx->stream;
  const size_t count = h.rows.size();
  HIP_TRY(ctx, md::to_device(d.rows, h.rows, st));
  HIP_TRY(ctx, md::to_device(d.in_off, h.in_off, st));
  HIP_TRY(ctx, md::to_device(d.in_len, h.in_len, st));
  HIP_TRY(ctx, md::to_device(d.out_off, h.out_off, st));
  HIP_TRY(ctx, md::to_device(d.out_cap, h.out_cap, st));
  int rc = md_inflate_batch_device(ctx, MD_FORMAT_ZLIB, count, d_pack, d.in_off, d.in_len, d_buf, d.out_off, d.out_cap, d.out_len, d.consumed, d.status,
                               nullptr);
  if (rc != MD_OK) return rc;
  if (verify) {
    HIP_TRY(ctx, md::to_device(d.p_off, h.p_off, st));
    HIP_TRY(ctx, md::to_device(d.p_len, h.p_len, st));
    MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)count, d_pack, d.p_off, d.p_len, d.crc, st));
  }
  MD_LAUNCH_TRY(ctx, md_launch_pk_verdict((uint32_t)count, d.rows, d.out_len, d.consumed, verify ? d.crc : nullptr, d.status, st));
  return MD_OK;
}

int pack_open(md_ctx *ctx, const uint8_t *pack, size_t pack_len, const uint8_t *idx, size_t idx_len, md_pack *P) {
  md_pack_index_info ii;
  int rc = md::pack::read_index(idx, idx_len, &ii, nullptr, 0);
  if (rc != MD_OK) return fail(ctx, rc, "md_pack_open: the idx");
  std::vector<md_pack_index_entry> ent((size_t)ii.n);
  rc = md::pack::read_index(idx, idx_len, &ii, ent.data(), ent.size());
  if (rc != MD_OK) return fail(ctx, rc, "md_pack_open: the idx");
  if ((rc = md::pack::pack_header_status(pack, pack_len)) != MD_OK)
    return fail(ctx, rc, rc == MD_INVALID_PACK ? "md_pack_open: no pack" : "md_pack_open: the pack's version is neither 2 nor 3");
  if (md::pack::be32(pack + 8) != ii.n) return fail(ctx, MD_INVALID_INDEX, "md_pack_open: the idx counts other objects than the pack");
  if (memcmp(pack + pack_len - 20, ii.pack_checksum, 20) != 0) return fail(ctx, MD_INVALID_INDEX, "md_pack_open: the idx belongs to another pack");
  const size_t n = (size_t)ii.n;
  if (n > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_open: too many objects");
  const uint64_t body_end = pack_len - md::pack::kPackTrailer;
  // the objects in pack order: object i is pack[off_i, the next offset)
  std::vector<std::pair<uint64_t, uint32_t>> order(n);
  for (size_t i = 0; i < n; i++) {
    if (ent[i].offset < md::pack::kPackHeader || ent[i].offset >= body_end) return fail(ctx, MD_INVALID_INDEX, "md_pack_open: an offset outside the pack");
    order[i] = {ent[i].offset, (uint32_t)i};
  }
  std::sort(order.begin(), order.end());
  std::vector<uint64_t> h_off(n), h_end(n), h_sorted(n);
  std::vector<uint32_t> h_sorted_obj(n), h_crc(n);
  std::vector<uint8_t> h_names(n * 20);
  for (size_t s = 0; s < n; s++) {
    if (s && order[s].first == order[s - 1].first) return fail(ctx, MD_INVALID_INDEX, "md_pack_open: two objects at one offset");
    const uint32_t i = order[s].second;
    h_sorted[s] = h_off[i] = order[s].first;
    h_sorted_obj[s] = i;
    h_end[i] = s + 1 < n ? order[s + 1].first : body_end;
  }
  for (size_t i = 0; i < n; i++) memcpy(&h_names[i * 20], ent[i].name, 20), h_crc[i] = ent[i].crc32;
  for (int b = 0; b < 256; b++) P->fan[b] = md::pack::be32(idx + 8 + 4 * b);
  memcpy(P->pack_checksum, ii.pack_checksum, 20);
  PackTableIn in;
  in.n = n, in.off = h_off.data(), in.end = h_end.data(), in.sorted_off = h_sorted.data(), in.sorted_obj = h_sorted_obj.data();
  in.names = in.obj_names = h_names.data(), in.n_names = n, in.crc = h_crc.data();  // (the idx's order is the names')
  return pack_table(ctx, pack, pack_len, in, false, P);
}
}  // namespace

int pack_table(md_ctx *ctx, const uint8_t *pack, size_t pack_len, const PackTableIn &in, bool resident, md_pack *P) {
  const size_t n = in.n;
  const uint64_t *h_off = in.off, *h_end = in.end;
  int rc = MD_OK;
  P->pack_len = pack_len;
  P->info = {};
  P->info.n = n;
  P->objs.assign(n, md_pack_object{});
  P->zoff.assign(n, 0);
  P->hsize.assign(n, 0);
  P->crc.resize(n);
  P->delta.assign(n, 0);
  if (n == 0) return MD_OK;

  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  md::pk::Table t = {};
  uint64_t *d_off = nullptr, *d_end = nullptr, *d_sorted = nullptr;
  uint32_t *d_sorted_obj = nullptr, *jump_b = nullptr, *links_b = nullptr, *d_root = nullptr, *d_depth = nullptr;
  uint8_t *d_names = nullptr;
  uint32_t *d_name_obj = nullptr;
  rc = carve(ctx, ctx->scratch[kPackDesc], "hipMalloc(pack table)", [&](md::Carver &c) {
    d_off = c.take<uint64_t>(n), d_end = c.take<uint64_t>(n), d_sorted = c.take<uint64_t>(n);
    t.hsize = c.take<uint64_t>(n), t.zoff = c.take<uint64_t>(n);
    d_sorted_obj = c.take<uint32_t>(n);
    t.base = c.take<uint32_t>(n), t.jump = c.take<uint32_t>(n), t.links = c.take<uint32_t>(n);
    jump_b = c.take<uint32_t>(n), links_b = c.take<uint32_t>(n), d_root = c.take<uint32_t>(n), d_depth = c.take<uint32_t>(n);
    t.status = c.take<int32_t>(n);
    t.type = c.take<uint8_t>(n);
    d_names = c.take<uint8_t>(in.n_names * 20);
    d_name_obj = c.take<uint32_t>(in.name_obj ? in.n_names : 0);
  });
  if (rc != MD_OK) return rc;
  t.n = n, t.pack_len = pack_len;
  t.off = d_off, t.end = d_end, t.sorted_off = d_sorted, t.sorted_obj = d_sorted_obj, t.names = d_names;
  t.n_names = in.n_names, t.name_obj = in.name_obj ? d_name_obj : nullptr;
  if (!resident && (rc = upload_host_in(ctx, pack, pack_len)) != MD_OK) return rc;
  const uint8_t *d_pack = ctx->scratch[kHostIn].as<uint8_t>();
  HIP_TRY(ctx, md::to_device(d_off, h_off, n, st));
  HIP_TRY(ctx, md::to_device(d_end, h_end, n, st));
  HIP_TRY(ctx, md::to_device(d_sorted, in.sorted_off, n, st));
  HIP_TRY(ctx, md::to_device(d_sorted_obj, in.sorted_obj, n, st));
  HIP_TRY(ctx, md::to_device(d_names, in.names, in.n_names * 20, st));
  if (in.name_obj) HIP_TRY(ctx, md::to_device(d_name_obj, in.name_obj, in.n_names, st));
  MD_LAUNCH_TRY(ctx, md_launch_pk_headers(&t, d_pack, st));
  // chains of at most n - 1 links: 2^rounds >= n brings every one to its root
  uint32_t *ja = t.jump, *la = t.links, *jb = jump_b, *lb = links_b;
  for (uint64_t reach = 1; reach < n; reach *= 2) {
    MD_LAUNCH_TRY(ctx, md_launch_pk_chain_step(n, ja, la, jb, lb, st));
    std::swap(ja, jb);
    std::swap(la, lb);
  }
  MD_LAUNCH_TRY(ctx, md_launch_pk_chain_finish(n, ja, la, d_root, d_depth, t.status, st));
  std::vector<uint32_t> base(n), root(n), depth(n);
  std::vector<int32_t> status(n);
  std::vector<uint8_t> type(n);
  HIP_TRY(ctx, md::to_host(P->hsize.data(), t.hsize, n, st));
  HIP_TRY(ctx, md::to_host(P->zoff.data(), t.zoff, n, st));
  HIP_TRY(ctx, md::to_host(base.data(), t.base, n, st));
  HIP_TRY(ctx, md::to_host(root.data(), d_root, n, st));
  HIP_TRY(ctx, md::to_host(depth.data(), d_depth, n, st));
  HIP_TRY(ctx, md::to_host(status.data(), t.status, n, st));
  HIP_TRY(ctx, md::to_host(type.data(), t.type, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));

  // -- the deltas' own sizes: their payloads through the decoder, in rounds of the workspace
  std::vector<uint64_t> result_size(n, 0), base_size(n, 0);
  std::vector<uint32_t> todo;
  for (size_t i = 0; i < n; i++) {
    if (status[i] == MD_OK && (h_end[i] - P->zoff[i] > MD_MAX_INFLATE_IN || P->hsize[i] > MD_MAX_STREAM)) status[i] = MD_E_INVALID_ARGUMENT;
    if (status[i] == MD_OK && base[i] != kNone) todo.push_back((uint32_t)i);
  }
  for (size_t t0 = 0; t0 < todo.size();) {
    size_t t1 = t0;
    uint64_t room = 0;
    RoundStreams h;
    for (; t1 < todo.size(); t1++) {
      const uint32_t i = todo[t1];
      if (t1 > t0 && room + slot_stride(P->hsize[i]) > ctx->pack_workspace) break;
      h.add(h_off[i], h_end[i] - h_off[i], P->zoff[i], P->hsize[i], in.crc ? in.crc[i] : 0, room);
      room += slot_stride(P->hsize[i]);
    }
    const size_t count = t1 - t0;
    RoundDesc d;
    rc = carve(ctx, ctx->scratch[kPackRound], "hipMalloc(pack round descriptors)", [&](md::Carver &c) { d.carve(&c, count, 0, 0); });
    if (rc != MD_OK) return rc;
    if ((rc = ctx->scratch[kPackScratch].reserve(ctx, room + 64, "hipMalloc(pack scratch)")) != MD_OK) return rc;
    uint8_t *d_buf = ctx->scratch[kPackScratch].as<uint8_t>();
    if ((rc = inflate_round(ctx, d, d_pack, d_buf, h, false)) != MD_OK) return rc;
    MD_LAUNCH_TRY(ctx, md_launch_pk_delta_sizes((uint32_t)count, d.rows, d_buf, d.out_off, d.base_size, d.result_size, d.status, st));
    std::vector<uint64_t> bs(count), rs(count);
    std::vector<int32_t> stt(count);
    HIP_TRY(ctx, md::to_host(bs.data(), d.base_size, count, st));
    HIP_TRY(ctx, md::to_host(rs.data(), d.result_size, count, st));
    HIP_TRY(ctx, md::to_host(stt.data(), d.status, count, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (size_t j = 0; j < count; j++) {
      const uint32_t i = todo[t0 + j];
      base_size[i] = bs[j], result_size[i] = rs[j], status[i] = stt[j];
      if (status[i] == MD_OK && rs[j] > MD_MAX_STREAM) status[i] = MD_E_INVALID_ARGUMENT;
    }
    t0 = t1;
  }

  // -- the last walk, in order of depth: a base's final size and status are known when its deltas are looked at
  uint32_t max_depth = 0;
  for (size_t i = 0; i < n; i++) max_depth = std::max(max_depth, depth[i]);
  std::vector<size_t> first((size_t)max_depth + 2, 0);
  for (size_t i = 0; i < n; i++) first[depth[i] + 1]++;
  for (size_t k = 1; k < first.size(); k++) first[k] += first[k - 1];
  std::vector<uint32_t> by_depth(n);
  {
    std::vector<size_t> at(first.begin(), first.end() - 1);
    for (size_t i = 0; i < n; i++) by_depth[at[depth[i]]++] = (uint32_t)i;
  }
  std::vector<uint64_t> size(n);
  for (uint32_t i : by_depth) {
    const bool linked = base[i] != kNone && depth[i] != 0;
    size[i] = linked ? result_size[i] : P->hsize[i];
    if (linked && status[i] == MD_OK) {
      if (status[base[i]] != MD_OK) status[i] = MD_INVALID_PACK_BASE;
      else if (base_size[i] != size[base[i]]) status[i] = MD_INVALID_DELTA;
    }
    if (status[i] != MD_OK) size[i] = 0;  // (what failed has no size: it takes no room in a read)
  }
  for (size_t i = 0; i < n; i++) {
    md_pack_object &o = P->objs[i];
    const uint32_t rt = type[root[i]];
    o.size = size[i];
    o.offset = h_off[i];
    o.packed_len = h_end[i] - h_off[i];
    o.base = base[i] == kNone ? MD_PACK_NO_BASE : base[i];
    o.depth = depth[i];
    o.type = rt >= 1 && rt <= 4 ? rt : 0;
    o.status = status[i];
    if (in.obj_names) memcpy(o.name, in.obj_names + i * 20, 20);
    P->crc[i] = in.crc ? in.crc[i] : 0;
    P->delta[i] = base[i] != kNone && depth[i] != 0;
    P->info.deltas += P->delta[i];
    P->info.max_depth = std::max<uint64_t>(P->info.max_depth, depth[i]);
    P->info.total_size += size[i];
    P->info.failed += status[i] != MD_OK;
  }
  return MD_OK;
}

namespace {
using md::PairTimers;

// one round of a read
struct ReadRound : RoundStreams {
  std::vector<uint32_t> obj;      // stream -> object
  std::vector<uint64_t> res_off;  // where the object's bytes stand in the end
  std::vector<Delta> deltas;      // sorted by depth
  std::vector<uint32_t> delta_depth;
  std::vector<Repeat> repeats;
  std::vector<int32_t> status;
  uint64_t scratch = 0;
  size_t selected = 0;
  // MD_PACK_VERIFY_NAME: the hash pass's messages (every object of the round where its bytes stand, its size and its root's
  // type), the idx's names, and what comes back: differs[slot] != 0, the SHA-1 is not the name
  std::vector<uint64_t> size;
  std::vector<uint8_t> type, names;
  std::vector<uint32_t> differs;
  std::vector<uint8_t> digest;  // md_pack_index_build: what the hash pass found, 20 bytes a slot
  Sha1Batch sha;
  std::vector<uint32_t> trees, others;  // md_pack_graph_build: the streams whose object is a tree / a commit or a tag
};

// md_pack_read (keep: the selected objects stand in dst, out_off[k + 1] says where) and md_pack_verify (!keep: they stand in
// the round's scratch like the bases, dst and out_off are null, nothing but the statuses comes back).  sink (with !keep:
// md_pack_index_build): the hash pass runs, an object whose name is not known yet gets what the pass found written to
// sink->names, one that has a name is compared as MD_PACK_VERIFY_NAME compares it; the pack is on the device already.
// links (with !keep: md_pack_graph_build): the link pass runs behind every round's last apply launch, over every object
// of the round where it stands.
// d_kept (with keep: md_pack_diff's levels): the device-resident form - the selected objects stay where the rounds put them,
// *d_kept + out_off[j], nothing of them is copied to the host and dst is not looked at; pack == null: it is in kHostIn already.
int pack_read(md_ctx *ctx, const md_pack *P, const uint8_t *pack, const uint64_t *select, size_t k, unsigned flags, bool keep, uint8_t *dst,
              size_t dst_cap, uint64_t *out_off, int32_t *status, md_pack_result *res, const PackNameSink *sink, PackLinkSink *links,
              const uint8_t **d_kept = nullptr) {
  const size_t n = P->objs.size();
  for (size_t j = 0; select && j < k; j++)
    if (select[j] >= n) return fail(ctx, MD_E_INVALID_ARGUMENT, "selected object out of range");
  const auto sel = [&](size_t j) { return select ? (size_t)select[j] : j; };
  const uint64_t need = keep ? md::running_offsets(k, out_off, [&](size_t j) { return P->objs[sel(j)].size; }) : 0;
  res->entries = k;
  res->written = need;
  if (need > dst_cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  ctx->pack_last = {};
  const bool names = (flags & MD_PACK_VERIFY_NAME) != 0 || sink;
  if (names) ctx->sha1_last = {}, ctx->sha1_span.pending = false;
  if (k == 0) return MD_OK;

  // -- the plan, from the table alone.  The buffer of a round: the output as it lies in dst, then the round's scratch.
  const uint64_t scratch0 = keep ? slot_stride(need) : 0, ws = ctx->pack_workspace;
  std::vector<uint32_t> stamp(n, kNone), slot_of(n, 0), sel_round(n, kNone), sel_slot(n, 0), first_at(n, kNone);
  std::vector<uint8_t> refused(n, 0);
  std::vector<ReadRound> rounds;
  std::vector<uint32_t> chain;
  const auto cost_of = [&](uint32_t s, uint32_t round) {  // the scratch that s and what of its chain the round lacks would take
    uint64_t cost = 0;
    chain.clear();
    for (uint32_t o = s;; o = (uint32_t)P->objs[o].base) {
      if (stamp[o] == round) break;
      chain.push_back(o);
      if (P->delta[o]) cost += slot_stride(P->hsize[o]);
      if (o != s || !keep) cost += slot_stride(P->objs[o].size);
      if (!P->delta[o]) break;
    }
    return cost;
  };
  for (size_t j = 0; j < k; j++) {
    const uint32_t s = (uint32_t)sel(j);
    if (P->objs[s].status != MD_OK || refused[s]) continue;
    if (first_at[s] != kNone) {  // selected before: copied from its first place when that round is through
      if (keep) rounds[sel_round[s]].repeats.push_back(Repeat{rounds[sel_round[s]].res_off[sel_slot[s]], out_off[j], P->objs[s].size});
      continue;
    }
    first_at[s] = (uint32_t)j;
    if (rounds.empty()) rounds.emplace_back();
    uint32_t r = (uint32_t)rounds.size() - 1;
    if (stamp[s] == r) {  // it is in this round's scratch, as another's base
      sel_round[s] = r, sel_slot[s] = slot_of[s];
      if (keep) rounds[r].repeats.push_back(Repeat{rounds[r].res_off[slot_of[s]], out_off[j], P->objs[s].size});
      continue;
    }
    uint64_t cost = cost_of(s, r);
    if (rounds[r].selected && (ws == 0 || rounds[r].scratch + cost > ws)) {
      rounds.emplace_back();
      r++;
      cost = cost_of(s, r);
    }
    if (ws != 0 && cost > ws) {
      refused[s] = 1;
      first_at[s] = kNone;
      continue;
    }
    ReadRound &R = rounds[r];
    R.selected++;
    for (size_t q = chain.size(); q-- > 0;) {  // bases first
      const uint32_t o = chain[q];
      const md_pack_object &ob = P->objs[o];
      const uint32_t slot = (uint32_t)R.obj.size();
      stamp[o] = r, slot_of[o] = slot;
      uint64_t place;  // of the object's bytes
      if (o == s && keep) place = out_off[j];
      else place = scratch0 + R.scratch, R.scratch += slot_stride(ob.size);
      uint64_t inflated = place;
      if (P->delta[o]) inflated = scratch0 + R.scratch, R.scratch += slot_stride(P->hsize[o]);
      R.obj.push_back(o);
      R.add(ob.offset, ob.packed_len, P->zoff[o], P->hsize[o], P->crc[o], inflated);
      R.res_off.push_back(place);
      if (P->delta[o]) {
        const uint32_t b = (uint32_t)ob.base;
        R.deltas.push_back(Delta{inflated, P->hsize[o], R.res_off[slot_of[b]], P->objs[b].size, place, ob.size, slot, slot_of[b]});
        R.delta_depth.push_back(ob.depth);
      }
    }
    sel_round[s] = r, sel_slot[s] = slot_of[s];
  }
  uint64_t max_scratch = 0;
  size_t max_count = 0, max_deltas = 0, max_repeats = 0;
  for (ReadRound &R : rounds) {
    // the levels one behind the other
    std::vector<size_t> perm(R.deltas.size());
    for (size_t q = 0; q < perm.size(); q++) perm[q] = q;
    std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return R.delta_depth[a] < R.delta_depth[b]; });
    std::vector<Delta> dl(perm.size());
    std::vector<uint32_t> dd(perm.size());
    for (size_t q = 0; q < perm.size(); q++) dl[q] = R.deltas[perm[q]], dd[q] = R.delta_depth[perm[q]];
    R.deltas.swap(dl), R.delta_depth.swap(dd);
    R.status.assign(R.obj.size(), 0);
    if (names) R.differs.assign(R.obj.size(), 0);
    if (names || links)
      for (uint32_t o : R.obj) {
        R.size.push_back(P->objs[o].size);
        R.type.push_back((uint8_t)P->objs[o].type);
        if (names) R.names.insert(R.names.end(), P->objs[o].name, P->objs[o].name + 20);
      }
    if (links)
      for (uint32_t q = 0; q < R.obj.size(); q++) {  // (an object of another type has no links: neither kernel sees it)
        if (R.type[q] == 2) R.trees.push_back(q);
        else if (R.type[q] == 1 || R.type[q] == 4) R.others.push_back(q);
      }
    max_scratch = std::max(max_scratch, R.scratch);
    max_count = std::max(max_count, R.obj.size());
    max_deltas = std::max(max_deltas, R.deltas.size());
    max_repeats = std::max(max_repeats, R.repeats.size());
  }
  if (max_count > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_read: too many objects in one round");

  // -- device memory: the pack, the buffer, one block of descriptors for the largest round
  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  int rc = sink || !pack ? MD_OK : upload_host_in(ctx, pack, P->pack_len);
  if (rc == MD_OK) rc = ctx->scratch[kHostOut].reserve(ctx, scratch0 + max_scratch + 64, "hipMalloc(pack output and scratch)");
  if (rc != MD_OK) return rc;
  RoundDesc d;
  rc = carve(ctx, ctx->scratch[kPackRound], "hipMalloc(pack round descriptors)", [&](md::Carver &c) { d.carve(&c, max_count, max_deltas, max_repeats, links ? max_count : 0); });
  if (rc != MD_OK) return rc;
  const uint8_t *d_pack = ctx->scratch[kHostIn].as<uint8_t>();
  uint8_t *d_buf = ctx->scratch[kHostOut].as<uint8_t>();
  md_pack_stats &stats = ctx->pack_last;
  stats.bytes_in = P->pack_len;
  const bool verify = (flags & MD_PACK_VERIFY_CRC) != 0;
  PairTimers timers, hash_timers, link_timers;
  md_sha1_stats &hashed = ctx->sha1_last;
  // -- the rounds, one behind the other on the context's stream: only the statuses come back
  for (ReadRound &R : rounds) {
    const size_t count = R.obj.size();
    if (count == 0) continue;
    if ((rc = inflate_round(ctx, d, d_pack, d_buf, R, verify)) != MD_OK) return rc;
    HIP_TRY(ctx, md::to_device(d.deltas, R.deltas, st));
    if (!R.deltas.empty()) timers.mark(st);
    for (size_t a = 0; a < R.deltas.size();) {  // one launch per level: the stream orders them
      size_t b = a + 1;
      while (b < R.deltas.size() && R.delta_depth[b] == R.delta_depth[a]) b++;
      MD_LAUNCH_TRY(ctx, md_launch_pk_apply((uint32_t)(b - a), d.deltas + a, d_buf, d.status, st));
      stats.apply_launches++;
      a = b;
    }
    if (!R.deltas.empty()) timers.mark(st);
    if (names) {  // behind the round's last apply launch: every object where it stands; the verdicts are the host's, below
      hash_timers.mark(st);
      if ((rc = sha1_enqueue(ctx, count, d_buf, R.res_off.data(), R.size.data(), R.type.data(), &R.sha, &hashed)) != MD_OK) return rc;
      HIP_TRY(ctx, md::to_device(R.sha.expect, R.names, st));
      MD_LAUNCH_TRY(ctx, md_launch_sha1_names((uint32_t)count, R.sha.digest, R.sha.expect, R.sha.differs, st));
      hash_timers.mark(st);
      HIP_TRY(ctx, md::to_host(R.differs.data(), R.sha.differs, count, st));
      if (sink) {
        R.digest.resize(count * kSha1Bytes);
        HIP_TRY(ctx, md::to_host(R.digest.data(), R.sha.digest, count * kSha1Bytes, st));
      }
    }
    if (links) {  // behind the round's last apply launch as well: what every commit, tree and tag of the round names
      HIP_TRY(ctx, md::to_device(d.l_off, R.res_off, st));
      HIP_TRY(ctx, md::to_device(d.l_size, R.size, st));
      HIP_TRY(ctx, md::to_device(d.l_type, R.type, st));
      HIP_TRY(ctx, md::to_device(d.l_obj, R.obj, st));
      HIP_TRY(ctx, md::to_device(d.l_trees, R.trees, st));
      HIP_TRY(ctx, md::to_device(d.l_others, R.others, st));
      md::pkg::Round rr = {(uint32_t)R.trees.size(), d.l_trees, d.l_obj, d.l_off, d.l_size, d.l_type, d.status};
      link_timers.mark(st);
      MD_LAUNCH_TRY(ctx, md_launch_pkg_tree_links(&rr, &links->links, d_buf, st));
      rr.count = (uint32_t)R.others.size(), rr.slot = d.l_others;
      MD_LAUNCH_TRY(ctx, md_launch_pkg_object_links(&rr, &links->links, d_buf, st));
      link_timers.mark(st);
      links->launches += !R.trees.empty() + !R.others.empty();
    }
    if (!R.repeats.empty()) {
      HIP_TRY(ctx, md::to_device(d.repeats, R.repeats, st));
      MD_LAUNCH_TRY(ctx, md_launch_pk_repeats((uint32_t)R.repeats.size(), d.repeats, d_buf, st));
    }
    HIP_TRY(ctx, md::to_host(R.status.data(), d.status, count, st));
    stats.rounds++;
    stats.inflate_launches++;
    stats.objects += count;
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  stats.apply_ns = timers.total_ns();
  if (links) links->device_ns = link_timers.total_ns();
  if (names) {
    hashed.device_ns = hash_timers.total_ns();
    // The names' verdicts, in the order of the header's rules: a status of its own stays; else a failed base; else the
    // name.  The deltas of a round are sorted by depth, so a base has its final status when its deltas are looked at.
    for (ReadRound &R : rounds) {
      if (sink)  // a name that is not known yet cannot differ
        for (size_t q = 0; q < R.obj.size(); q++)
          if (!sink->known[R.obj[q]]) R.differs[q] = 0;
      for (size_t q = 0; q < R.obj.size(); q++)
        if (!P->delta[R.obj[q]] && R.status[q] == MD_OK && R.differs[q]) R.status[q] = MD_INVALID_CHECKSUM;
      for (const Delta &dl : R.deltas)
        if (R.status[dl.self] == MD_OK) {
          if (R.status[dl.base_slot] != MD_OK) R.status[dl.self] = MD_INVALID_PACK_BASE;
          else if (R.differs[dl.self]) R.status[dl.self] = MD_INVALID_CHECKSUM;
        }
    }
  }
  if (sink)
    for (const ReadRound &R : rounds)
      for (size_t q = 0; q < R.obj.size(); q++)
        if (R.status[q] == MD_OK && !sink->known[R.obj[q]]) memcpy(sink->names + (size_t)R.obj[q] * kSha1Bytes, &R.digest[q * kSha1Bytes], kSha1Bytes), sink->named[R.obj[q]] = 1;
  if (d_kept) *d_kept = d_buf;
  else if (keep && need) HIP_TRY(ctx, hipMemcpy(dst, d_buf, (size_t)need, hipMemcpyDeviceToHost));
  for (size_t j = 0; j < k; j++) {
    const uint32_t s = (uint32_t)sel(j);
    status[j] = P->objs[s].status != MD_OK ? P->objs[s].status : refused[s] ? MD_E_OUT_OF_MEMORY : rounds[sel_round[s]].status[sel_slot[s]];
    res->failed += status[j] != MD_OK;
  }
  return MD_OK;
}
}  // namespace

int pack_verify_names(md_ctx *ctx, const md_pack *P, const uint64_t *select, size_t k, int32_t *status, md_pack_result *res, const PackNameSink *sink) {
  return pack_read(ctx, P, nullptr, select, k, 0, false, nullptr, 0, nullptr, status, res, sink, nullptr);
}

int pack_link_rounds(md_ctx *ctx, const md_pack *P, const uint8_t *pack, const uint64_t *select, size_t k, unsigned flags, int32_t *status,
                     md_pack_result *res, PackLinkSink *links) {
  return pack_read(ctx, P, pack, select, k, flags, false, nullptr, 0, nullptr, status, res, nullptr, links);
}

int pack_read_resident(md_ctx *ctx, const md_pack *P, const uint8_t *pack, const uint64_t *select, size_t k, uint64_t *out_off, int32_t *status,
                       md_pack_result *res, const uint8_t **d_objs) {
  return pack_read(ctx, P, pack, select, k, 0, true, nullptr, SIZE_MAX, out_off, status, res, nullptr, nullptr, d_objs);
}

int md_pack_index(const uint8_t *idx, size_t idx_len, md_pack_index_info *info, md_pack_index_entry *entries, size_t cap) {
  if (!idx || !info || (cap && !entries)) return MD_E_INVALID_ARGUMENT;
  return md::pack::read_index(idx, idx_len, info, entries, cap);
}

int md_pack_open(md_ctx *ctx, const uint8_t *pack, size_t pack_len, const uint8_t *idx, size_t idx_len, md_pack **p) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!p) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  *p = nullptr;
  if (!pack || !idx) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  md_pack *P = new (std::nothrow) md_pack();
  if (!P) return fail(ctx, MD_E_OUT_OF_MEMORY, "host memory for the pack's table");
  const int rc = no_bad_alloc(ctx, "host memory for the pack's table", [&] { return pack_open(ctx, pack, pack_len, idx, idx_len, P); });
  if (rc != MD_OK) {
    delete P;
    return rc;
  }
  *p = P;
  return MD_OK;
}

int md_pack_get(const md_pack *p, md_pack_info *info) {
  if (!p || !info) return MD_E_INVALID_ARGUMENT;
  *info = p->info;
  return MD_OK;
}

int md_pack_objects(const md_pack *p, md_pack_object *objs, size_t cap) {
  if (!p || (cap && !objs)) return MD_E_INVALID_ARGUMENT;
  const size_t k = std::min(cap, p->objs.size());
  if (k) memcpy(objs, p->objs.data(), k * sizeof(md_pack_object));
  return MD_OK;
}

int64_t md_pack_find(const md_pack *p, const uint8_t *name20) {
  if (!p || !name20 || p->objs.empty()) return -1;
  return md::pack::find_name(p->objs[0].name, sizeof(md_pack_object), p->fan, name20);
}

void md_pack_free(md_pack *p) { delete p; }

int md_pack_last(const md_ctx *ctx, md_pack_stats *stats) {
  if (!ctx || !stats) return MD_E_INVALID_ARGUMENT;
  *stats = ctx->pack_last;
  return MD_OK;
}

// the checks md_pack_read and md_pack_verify share (pointers: those of the caller's own are there); *k = the objects of the call
static int pack_checks(md_ctx *ctx, bool verify, bool pointers, const md_pack *p, const uint8_t *pack, size_t pack_len, const uint64_t *select,
                       size_t nselect, unsigned flags, const int32_t *status, md_pack_result *res, size_t *k) {
  if (!p || !pack || !res || !pointers) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  memset(res, 0, sizeof *res);
  if (flags & ~(MD_PACK_VERIFY_CRC | MD_PACK_VERIFY_NAME))
    return fail(ctx, MD_E_INVALID_ARGUMENT, verify ? "md_pack_verify: unknown flag" : "md_pack_read: unknown flag");
  if (pack_len != p->pack_len || memcmp(pack + pack_len - 20, p->pack_checksum, 20) != 0)
    return fail(ctx, MD_INVALID_INDEX, verify ? "md_pack_verify: the table belongs to another pack" : "md_pack_read: the table belongs to another pack");
  *k = select ? nselect : p->objs.size();
  if (*k > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many objects in one call");
  if (*k && !status) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  return MD_OK;
}

int md_pack_read(md_ctx *ctx, const md_pack *p, const uint8_t *pack, size_t pack_len, const uint64_t *select, size_t nselect, unsigned flags,
                 uint8_t *dst, size_t dst_cap, uint64_t *out_off, int32_t *status, md_pack_result *res) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  size_t k = 0;
  const int rc = pack_checks(ctx, false, out_off && (dst || !dst_cap), p, pack, pack_len, select, nselect, flags, status, res, &k);
  if (rc != MD_OK) return rc;
  return no_bad_alloc(ctx, "host memory for the read's plan",
                      [&] { return pack_read(ctx, p, pack, select, k, flags, true, dst, dst_cap, out_off, status, res, nullptr, nullptr); });
}

int md_pack_verify(md_ctx *ctx, const md_pack *p, const uint8_t *pack, size_t pack_len, const uint64_t *select, size_t nselect, unsigned flags,
                   int32_t *status, md_pack_result *res) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  size_t k = 0;
  const int rc = pack_checks(ctx, true, true, p, pack, pack_len, select, nselect, flags, status, res, &k);
  if (rc != MD_OK) return rc;
  return no_bad_alloc(ctx, "host memory for the verification's plan",
                      [&] { return pack_read(ctx, p, pack, select, k, flags, false, nullptr, 0, nullptr, status, res, nullptr, nullptr); });
}
