// capi_pack_build.cpp — the idx of a git pack from the pack alone (mdeflate.h: md_pack_index_write, md_pack_index_build,
// md_pack_build_last).  The candidates, their size query and everything an object is decoded, applied and hashed
// with are the device's (pack_build_kernels.hip, inflate_count.hip, pack_kernels.hip, sha1_kernels.hip); the walk over the
// candidates, the order of the generations, the sort of the names and the idx's bytes are the host's (pack_build.hpp).
// The table of a generation is md_pack_open's (pack_table) with the names known so far, its read md_pack_verify's
// (pack_verify_names) with a hash pass that writes the names it has not got yet.
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "pack_build.hpp"

namespace {

// what the device knows of every candidate, read back (z ascending)
struct CandidateTable {
  std::vector<uint64_t> z, consumed, out_len;
  std::vector<int32_t> status;
};

// Mark, scan, compact, the inputs and ONE size query over every candidate of the pack in kHostIn; with check_trailer the
// host hashes the pack while the device counts.  *trailer_ok is written with check_trailer alone.
int candidates(md_ctx *ctx, const uint8_t *pack, uint64_t pack_len, bool check_trailer, CandidateTable *t, bool *trailer_ok) {
  hipStream_t st = ctx->stream;
  const uint8_t *d_pack = ctx->scratch[kHostIn].as<uint8_t>();
  const uint64_t end = pack_len - md::pkb::kPackTrailer;
  const uint64_t nspans = (pack_len + md::gzm::kMarkSpanBytes - 1) / md::gzm::kMarkSpanBytes, nwords = (pack_len + 31) / 32;
  uint32_t *bits = nullptr, *cnt = nullptr;
  uint64_t *base = nullptr;
  int rc = carve(ctx, ctx->scratch[kGzmWs], "hipMalloc(pack candidates' bitmap)", [&](md::Carver &ws) {
    bits = ws.take<uint32_t>(nwords), cnt = ws.take<uint32_t>(nspans);
    base = ws.take<uint64_t>(nspans + 1);
  });
  if (rc != MD_OK) return rc;
  MD_LAUNCH_TRY(ctx, md_launch_pkb_mark(d_pack, pack_len, md::pkb::kPackHeader, end - md::pkb::kCandidateMin, bits, cnt, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan32(cnt, nspans, base, st));
  uint64_t C = 0;
  HIP_TRY(ctx, md::to_host(&C, base + nspans, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (C > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_index_build: too many candidates");
  uint64_t *cpos = nullptr, *in_len = nullptr, *out_len = nullptr, *consumed = nullptr;
  int32_t *status = nullptr;
  if (C) {
    rc = ctx->scratch[kGzmCand].reserve(ctx, (size_t)C * sizeof(uint64_t), "hipMalloc(pack candidates)");
    if (rc != MD_OK) return rc;
    cpos = ctx->scratch[kGzmCand].as<uint64_t>();
    rc = carve(ctx, ctx->scratch[kGzmDesc], "hipMalloc(pack candidates' descriptors)", [&](md::Carver &c) {
      in_len = c.take<uint64_t>(C), out_len = c.take<uint64_t>(C), consumed = c.take<uint64_t>(C);
      status = c.take<int32_t>(C);
    });
    if (rc != MD_OK) return rc;
    MD_LAUNCH_TRY(ctx, md_launch_gzs_compact(pack_len, bits, base, cpos, st));
    MD_LAUNCH_TRY(ctx, md_launch_pkb_inputs(C, cpos, end, in_len, st));
    rc = md_inflate_sizes_batch_device(ctx, MD_FORMAT_ZLIB, (size_t)C, d_pack, cpos, in_len, out_len, consumed, status);
    if (rc != MD_OK) return rc;
  }
  t->z.resize((size_t)C), t->consumed.resize((size_t)C), t->out_len.resize((size_t)C), t->status.resize((size_t)C);
  HIP_TRY(ctx, md::to_host(t->z.data(), cpos, (size_t)C, st));
  HIP_TRY(ctx, md::to_host(t->consumed.data(), consumed, (size_t)C, st));
  HIP_TRY(ctx, md::to_host(t->out_len.data(), out_len, (size_t)C, st));
  HIP_TRY(ctx, md::to_host(t->status.data(), status, (size_t)C, st));
  if (check_trailer) {  // one serial message: the host's, under the device's count
    uint8_t digest[20];
    md::sha::sha1_of(pack, (size_t)end, digest);
    *trailer_ok = memcmp(digest, pack + end, 20) == 0;
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return MD_OK;
}

int index_build(md_ctx *ctx, const uint8_t *pack, size_t pack_len, unsigned flags, uint8_t *idx, size_t idx_cap, uint64_t *offsets,
                int32_t *status, size_t cap, md_pack_build_result *res) {
  md_pack_build_stats &stats = ctx->pack_build_last;
  stats = {};
  stats.bytes_in = pack_len;
  const uint64_t end = pack_len - md::pkb::kPackTrailer;
  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  int rc = upload_host_in(ctx, pack, pack_len);
  if (rc != MD_OK) return rc;
  const uint8_t *d_pack = ctx->scratch[kHostIn].as<uint8_t>();

  // -- where the objects begin
  CandidateTable t;
  bool trailer_ok = true;
  if ((rc = candidates(ctx, pack, pack_len, (flags & MD_PACK_BUILD_CHECK_TRAILER) != 0, &t, &trailer_ok)) != MD_OK) return rc;
  stats.candidates = t.z.size();
  if (!trailer_ok) {
    res->bad_offset = end;
    return fail(ctx, MD_INVALID_CHECKSUM, "md_pack_index_build: the pack's trailer is not the SHA-1 of what is in front of it");
  }
  md::pkb::Candidates c;
  c.C = t.z.size(), c.z = t.z.data(), c.consumed = t.consumed.data(), c.out_len = t.out_len.data(), c.status = t.status.data();
  md::pkb::Walk w;
  if (md::pkb::walk(pack, pack_len, c, &w) != MD_OK) {
    res->bad_offset = w.bad_offset, res->bad_status = w.bad_status;
    return fail(ctx, MD_INVALID_PACK, "md_pack_index_build: the chain of objects breaks (md_pack_build_result::bad_offset)");
  }
  const size_t n = w.off.size();
  uint64_t escapes = 0;
  for (uint64_t o : w.off) escapes += o > 0x7fffffffull;
  res->n = n;
  res->idx_len = md::pkb::index_len(n, escapes);
  for (size_t i = 0; i < n && i < cap; i++) offsets[i] = w.off[i];
  if (res->idx_len > idx_cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  if (n > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_index_build: too many objects");
  std::vector<md_pack_index_entry> ent(n);
  size_t written = 0;
  if (n == 0) return md::pkb::write_index(ent.data(), 0, pack + end, idx, idx_cap, &written);

  // -- the CRC-32 of every object's packed bytes: one launch
  std::vector<uint64_t> h_end(n), p_len(n);
  std::vector<uint32_t> h_crc(n), iota(n);
  for (size_t i = 0; i < n; i++) h_end[i] = i + 1 < n ? w.off[i + 1] : end, p_len[i] = h_end[i] - w.off[i], iota[i] = (uint32_t)i;
  {
    uint64_t *d_off = nullptr, *d_len = nullptr;
    uint32_t *d_crc = nullptr;
    rc = carve(ctx, ctx->scratch[kPackRound], "hipMalloc(pack CRC descriptors)",
               [&](md::Carver &cv) { d_off = cv.take<uint64_t>(n), d_len = cv.take<uint64_t>(n), d_crc = cv.take<uint32_t>(n); });
    if (rc != MD_OK) return rc;
    HIP_TRY(ctx, md::to_device(d_off, w.off, st));
    HIP_TRY(ctx, md::to_device(d_len, p_len, st));
    MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)n, d_pack, d_off, d_len, d_crc, st));
    HIP_TRY(ctx, md::to_host(h_crc.data(), d_crc, n, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }

  // -- the generations: the table with the names known so far, then a read of what it says can be decoded and has no
  // verdict yet; what the read names may be the base some REF_DELTA waits for
  std::vector<uint8_t> names(n * 20, 0), known(n, 0), named(n, 0), done(n, 0), sorted_names;
  std::vector<int32_t> verdict(n, MD_OK), table_status(n, MD_OK);
  std::vector<uint64_t> hsize;
  std::vector<uint32_t> name_obj;
  std::vector<uint64_t> select;
  for (;;) {
    name_obj.clear();
    for (size_t i = 0; i < n; i++)
      if (known[i]) name_obj.push_back((uint32_t)i);
    std::sort(name_obj.begin(), name_obj.end(), [&](uint32_t a, uint32_t b) {
      const int cmp = memcmp(&names[(size_t)a * 20], &names[(size_t)b * 20], 20);
      return cmp != 0 ? cmp < 0 : a < b;
    });
    sorted_names.resize(name_obj.size() * 20);
    for (size_t k = 0; k < name_obj.size(); k++) memcpy(&sorted_names[k * 20], &names[(size_t)name_obj[k] * 20], 20);
    PackTableIn in;
    in.n = n, in.off = w.off.data(), in.end = h_end.data(), in.sorted_off = w.off.data(), in.sorted_obj = iota.data();
    in.names = sorted_names.data(), in.n_names = name_obj.size(), in.name_obj = name_obj.data();
    in.obj_names = names.data(), in.crc = h_crc.data();
    md_pack P;
    memcpy(P.pack_checksum, pack + end, 20);
    if ((rc = pack_table(ctx, pack, pack_len, in, true, &P)) != MD_OK) return rc;
    select.clear();
    bool waiting = false;
    for (size_t i = 0; i < n; i++) {
      table_status[i] = P.objs[i].status;
      if (done[i]) continue;
      if (table_status[i] == MD_OK) select.push_back(i);
      else waiting |= table_status[i] == MD_PACK_MISSING_BASE || table_status[i] == MD_INVALID_PACK_BASE;
    }
    hsize = P.hsize;
    if (select.empty()) break;
    stats.generations++;
    std::vector<int32_t> got(select.size(), MD_OK);
    md_pack_result rr = {};
    PackNameSink sink;
    sink.known = known.data(), sink.names = names.data(), sink.named = named.data();
    if ((rc = pack_verify_names(ctx, &P, select.data(), select.size(), got.data(), &rr, &sink)) != MD_OK) return rc;
    const md_pack_stats &ps = ctx->pack_last;
    stats.rounds += ps.rounds, stats.inflate_launches += ps.inflate_launches, stats.apply_launches += ps.apply_launches, stats.objects += ps.objects;
    for (size_t j = 0; j < select.size(); j++) done[select[j]] = 1, verdict[select[j]] = got[j];
    size_t fresh = 0;
    for (size_t i = 0; i < n; i++)
      if (named[i] && !known[i]) known[i] = 1, fresh++;
    if (!fresh || !waiting) break;  // nothing a pending REF_DELTA could find, or none pending
  }

  // -- the verdicts, in pack order
  for (size_t i = 0; i < n; i++) {
    if (!done[i]) verdict[i] = w.inflated[i] != hsize[i] ? MD_INVALID_SIZE : table_status[i];
  }
  bool sound = true;
  for (size_t i = 0; i < n && sound; i++) sound = verdict[i] == MD_OK;
  if (sound) {  // the idx writer sorts the names: it is the one that meets two equal ones
    for (size_t i = 0; i < n; i++) {
      ent[i].offset = w.off[i], ent[i].crc32 = h_crc[i];
      memcpy(ent[i].name, &names[i * 20], 20);
    }
    rc = md::pkb::write_index(ent.data(), n, pack + end, idx, idx_cap, &written);
    if (rc == MD_OK)
      for (size_t i = 0; i < n && i < cap; i++) status[i] = MD_OK;
    if (rc != MD_INVALID_INDEX) return rc;
  }
  {  // of two objects with one name the later is refused: the idx's names ascend strictly
    std::vector<uint32_t> by_name;
    for (size_t i = 0; i < n; i++)
      if (verdict[i] == MD_OK) by_name.push_back((uint32_t)i);
    std::sort(by_name.begin(), by_name.end(), [&](uint32_t a, uint32_t b) {
      const int cmp = memcmp(&names[(size_t)a * 20], &names[(size_t)b * 20], 20);
      return cmp != 0 ? cmp < 0 : a < b;
    });
    for (size_t k = 1; k < by_name.size(); k++)
      if (memcmp(&names[(size_t)by_name[k - 1] * 20], &names[(size_t)by_name[k] * 20], 20) == 0) verdict[by_name[k]] = MD_INVALID_PACK;
  }
  int first = MD_OK;
  for (size_t i = 0; i < n; i++) {
    if (i < cap) status[i] = verdict[i];
    if (verdict[i] == MD_OK) continue;
    if (res->failed++ == 0) first = verdict[i], res->bad_offset = w.off[i];
  }
  return fail(ctx, first, "md_pack_index_build: an object of the pack failed (md_pack_build_result::bad_offset)");
}
}  // namespace

int md_pack_index_write(const md_pack_index_entry *entries, size_t n, const uint8_t pack_checksum[20], uint8_t *idx, size_t idx_cap,
                        size_t *idx_len) {
  if ((n && !entries) || !pack_checksum || !idx_len || (idx_cap && !idx)) return MD_E_INVALID_ARGUMENT;
  try {
    return md::pkb::write_index(entries, n, pack_checksum, idx, idx_cap, idx_len);
  } catch (const std::bad_alloc &) {
    return MD_E_OUT_OF_MEMORY;
  }
}

int md_pack_index_build(md_ctx *ctx, const uint8_t *pack, size_t pack_len, unsigned flags, uint8_t *idx, size_t idx_cap, uint64_t *offsets,
                        int32_t *status, size_t cap, md_pack_build_result *res) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!pack || !res || (idx_cap && !idx) || (cap && (!offsets || !status))) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  memset(res, 0, sizeof *res);
  res->bad_offset = MD_PACK_NO_BASE;
  if (flags & ~MD_PACK_BUILD_CHECK_TRAILER) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_pack_index_build: unknown flag");
  if (const int rc = md::pack::pack_header_status(pack, pack_len))
    return fail(ctx, rc, rc == MD_INVALID_PACK ? "md_pack_index_build: no pack" : "md_pack_index_build: the pack's version is neither 2 nor 3");
  return no_bad_alloc(ctx, "host memory for the pack's objects",
                      [&] { return index_build(ctx, pack, pack_len, flags, idx, idx_cap, offsets, status, cap, res); });
}

int md_pack_build_last(const md_ctx *ctx, md_pack_build_stats *stats) {
  if (!ctx || !stats) return MD_E_INVALID_ARGUMENT;
  *stats = ctx->pack_build_last;
  return MD_OK;
}
