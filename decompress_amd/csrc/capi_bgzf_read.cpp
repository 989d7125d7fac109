// capi_bgzf_read.cpp — random access to a blocked GZip file (mdeflate.h: md_bgzf_index_*, md_bgzf_read*): the index object
// (bgzf_index.hpp), and the read of any set of byte ranges or virtual offsets, planned on the host from the index alone and
// run as one inflate launch a round (bgzf_read.hip has the kernels).
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "bgzf_index.hpp"
#include "ctx.hpp"

int md_bgzf_index_build(md_ctx *ctx, const uint8_t *src, size_t src_len, md_bgzf_index **idx) {
  if (idx) *idx = nullptr;
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!idx || (!src && src_len)) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_bgzf_index_build: null pointer");
  return no_bad_alloc(ctx, "md_bgzf_index_build", [&]() -> int {
    md_bgzf_index *x = new md_bgzf_index();
    std::unique_ptr<md_bgzf_index> hold(x);
    x->src_len = src_len;
    if (src_len) {
      MD_ON_DEVICE(ctx);
      int rc = upload_host_in(ctx, src, src_len);
      if (rc != MD_OK) return rc;
      bool indexed = false;
      GzmIndex ix;
      rc = gzm_index(ctx, ctx->scratch[kHostIn].as<const uint8_t>(), src_len, &indexed, &ix);
      if (rc != MD_OK) return rc;
      if (!indexed) return MD_INVALID_INDEX;
      const size_t M = (size_t)ix.M;
      uint64_t last_len = 0;
      x->c_off.assign(M + 1, 0);
      x->u_off.assign(M + 1, 0);
      HIP_TRY(ctx, md::to_host(x->c_off.data(), ix.mpos, M, ctx->stream));
      HIP_TRY(ctx, md::to_host(x->u_off.data(), ix.out_off, M + 1, ctx->stream));
      HIP_TRY(ctx, md::to_host(&last_len, ix.mlen + (M - 1), 1, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      x->c_off[M] = x->c_off[M - 1] + last_len;
    }
    *idx = hold.release();
    return MD_OK;
  });
}

int md_bgzf_index_from_gzi(const uint8_t *gzi, size_t gzi_len, const uint8_t *src, size_t src_len, md_bgzf_index **idx) {
  if (idx) *idx = nullptr;
  if (!idx || (!gzi && gzi_len) || (!src && src_len)) return MD_E_INVALID_ARGUMENT;
  return md::bgzf::from_gzi(gzi, gzi_len, src, src_len, idx);
}

size_t md_bgzf_index_gzi_size(const md_bgzf_index *idx) { return idx ? md::bgzf::gzi_size(idx) : 0; }

int md_bgzf_index_to_gzi(const md_bgzf_index *idx, uint8_t *buf, size_t cap, size_t *len) {
  if (!idx || !len || (!buf && cap)) return MD_E_INVALID_ARGUMENT;
  *len = md::bgzf::gzi_size(idx);
  if (*len > cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  md::bgzf::to_gzi(idx, buf);
  return MD_OK;
}

int md_bgzf_index_get(const md_bgzf_index *idx, md_bgzf_index_info *info) {
  if (!idx || !info) return MD_E_INVALID_ARGUMENT;
  info->src_len = idx->src_len;
  info->members = idx->members();
  info->size = idx->size();
  return MD_OK;
}

int md_bgzf_index_entries(const md_bgzf_index *idx, uint64_t *c_off, uint64_t *u_off, size_t cap) {
  if (!idx || (cap && (!c_off || !u_off))) return MD_E_INVALID_ARGUMENT;
  const size_t k = std::min(cap, idx->c_off.size());
  if (k) {
    memcpy(c_off, idx->c_off.data(), k * 8);
    memcpy(u_off, idx->u_off.data(), k * 8);
  }
  return MD_OK;
}

void md_bgzf_index_free(md_bgzf_index *idx) { delete idx; }

int md_bgzf_read_last(const md_ctx *ctx, md_bgzf_read_stats *stats) {
  if (!ctx || !stats) return MD_E_INVALID_ARGUMENT;
  *stats = ctx->bgr_last;
  return MD_OK;
}

namespace {
// the member that holds byte x of the output (x < size): the last k with u_off[k] <= x - never an empty one
inline size_t member_of(const std::vector<uint64_t> &u_off, uint64_t x) {
  return (size_t)(std::upper_bound(u_off.begin(), u_off.end(), x) - u_off.begin()) - 1;
}
struct RoundPlan {
  size_t t0, t1;           // its members, as positions in the list of touched members
  uint64_t in_bytes, slot_bytes, longest;
  size_t id0, id1;         // its ranges, as positions in the list of (round, range) pairs
};
}  // namespace

// The read of n ranges that passed the call-level checks; status[i] != MD_OK on entry: range i is not read (a virtual
// offset the index does not know).
static int bgzf_read_ranges(md_ctx *ctx, const md_bgzf_index *idx, const uint8_t *src, size_t n, const uint64_t *off, const uint64_t *len,
                            uint8_t *dst, const uint64_t *dst_off, int32_t *status) {
  md_bgzf_read_stats &stats = ctx->bgr_last;
  const std::vector<uint64_t> &c_off = idx->c_off, &u_off = idx->u_off;
  // -- the plan, from the index alone and at the cost of the ranges and the members they touch, not of the file's members:
  // per range its first and last member with output (a binary search each); the spans, sorted and merged, give every
  // touched member once, in member order, however many ranges touch it
  std::vector<size_t> first_m(n), last_m(n);
  std::vector<std::pair<size_t, size_t>> spans;
  uint64_t room = 0;  // bytes of dst the ranges reach
  for (size_t i = 0; i < n; i++) {
    if (len[i] == 0 || status[i] != MD_OK) continue;
    first_m[i] = member_of(u_off, off[i]);
    last_m[i] = member_of(u_off, off[i] + len[i] - 1);
    spans.push_back({first_m[i], last_m[i]});
    room = std::max(room, dst_off[i] + len[i]);
  }
  if (spans.empty()) return MD_OK;
  std::sort(spans.begin(), spans.end());
  std::vector<size_t> touched;
  size_t next = 0;  // the first member no span has covered yet
  for (const auto &sp : spans)
    for (size_t k = std::max(next, sp.first); k <= sp.second; next = ++k)
      if (u_off[k + 1] > u_off[k]) touched.push_back(k);
  // (a range's first and last member have output, so both are in the list)
  const auto t_of = [&](size_t k) { return (size_t)(std::lower_bound(touched.begin(), touched.end(), k) - touched.begin()); };
  const size_t T = touched.size();
  if (T > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_bgzf_read: too many members in one call");
  // -- rounds: as many touched members as the workspace holds (packed input + slots), the first always
  std::vector<uint64_t> h_mpos(T), h_mlen(T), h_slot(T), h_cap(T), h_u0(T);
  std::vector<RoundPlan> rounds;
  for (size_t t = 0; t < T;) {
    RoundPlan r{t, t, 0, 0, 0, 0, 0};
    for (; r.t1 < T; r.t1++) {
      const size_t k = touched[r.t1];
      const uint64_t ml = c_off[k + 1] - c_off[k], cap = u_off[k + 1] - u_off[k];
      if (r.t1 > r.t0 && r.in_bytes + ml + r.slot_bytes + md::bgr::slot_stride(cap) > ctx->bgr_workspace) break;
      h_mpos[r.t1] = r.in_bytes;
      h_mlen[r.t1] = ml;
      h_slot[r.t1] = r.slot_bytes;
      h_cap[r.t1] = cap;
      h_u0[r.t1] = u_off[k];
      r.in_bytes += ml;
      r.slot_bytes += md::bgr::slot_stride(cap);
    }
    rounds.push_back(r);
    t = r.t1;
  }
  // the ranges of every round: those with bytes in one of its members
  std::vector<uint32_t> h_ids;
  {
    std::vector<size_t> round_of(T);
    for (size_t q = 0; q < rounds.size(); q++)
      for (size_t t = rounds[q].t0; t < rounds[q].t1; t++) round_of[t] = q;
    std::vector<std::vector<uint32_t>> per(rounds.size());
    for (size_t i = 0; i < n; i++) {
      if (len[i] == 0 || status[i] != MD_OK) continue;
      const size_t qa = round_of[t_of(first_m[i])], qb = round_of[t_of(last_m[i])];
      for (size_t q = qa; q <= qb; q++) {
        RoundPlan &r = rounds[q];
        const uint64_t lo = h_u0[r.t0], hi = h_u0[r.t1 - 1] + h_cap[r.t1 - 1];
        r.longest = std::max(r.longest, std::min(off[i] + len[i], hi) - std::max(off[i], lo));
        per[q].push_back((uint32_t)i);
      }
    }
    for (size_t q = 0; q < rounds.size(); q++) {
      rounds[q].id0 = h_ids.size();
      h_ids.insert(h_ids.end(), per[q].begin(), per[q].end());
      rounds[q].id1 = h_ids.size();
    }
  }
  uint64_t max_in = 0, max_slots = 0;
  for (const RoundPlan &r : rounds) max_in = std::max(max_in, r.in_bytes), max_slots = std::max(max_slots, r.slot_bytes);
  // -- device memory: blob, slots, the ranges' bytes as they lie in dst, and one block of tables
  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  int rc = ctx->scratch[kBgrIn].reserve(ctx, max_in + 64, "hipMalloc(bgzf read input)");
  if (rc == MD_OK) rc = ctx->scratch[kBgrSlots].reserve(ctx, max_slots + 64, "hipMalloc(bgzf read slots)");
  if (rc == MD_OK) rc = ctx->scratch[kHostOut].reserve(ctx, room + 64, "hipMalloc(host path output)");
  if (rc != MD_OK) return rc;
  uint64_t *d_mpos = nullptr, *d_mlen = nullptr, *d_slot = nullptr, *d_cap = nullptr, *d_u0 = nullptr, *d_body_off = nullptr, *d_body_len = nullptr,
           *d_isize = nullptr, *d_out_len = nullptr, *d_consumed = nullptr, *d_inf_consumed = nullptr, *d_off = nullptr, *d_len = nullptr,
           *d_dst_off = nullptr;
  int32_t *d_hstatus = nullptr, *d_status = nullptr, *d_inf_status = nullptr, *d_verdict = nullptr, *d_rstatus = nullptr;
  uint32_t *d_ids = nullptr;
  rc = carve(ctx, ctx->scratch[kGzmDesc], "hipMalloc(member descriptors)", [&](md::Carver &c) {
    uint64_t **m64[11] = {&d_mpos, &d_mlen, &d_slot, &d_cap, &d_u0, &d_body_off, &d_body_len, &d_isize, &d_out_len, &d_consumed, &d_inf_consumed};
    for (uint64_t **p : m64) *p = c.take<uint64_t>(T);
    d_off = c.take<uint64_t>(n), d_len = c.take<uint64_t>(n), d_dst_off = c.take<uint64_t>(n);
    int32_t **m32[4] = {&d_hstatus, &d_status, &d_inf_status, &d_verdict};
    for (int32_t **p : m32) *p = c.take<int32_t>(T);
    d_rstatus = c.take<int32_t>(n);
    d_ids = c.take<uint32_t>(h_ids.size());
  }, 64);
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_device(d_mpos, h_mpos, st));
  HIP_TRY(ctx, md::to_device(d_mlen, h_mlen, st));
  HIP_TRY(ctx, md::to_device(d_slot, h_slot, st));
  HIP_TRY(ctx, md::to_device(d_cap, h_cap, st));
  HIP_TRY(ctx, md::to_device(d_u0, h_u0, st));
  HIP_TRY(ctx, md::to_device(d_off, off, n, st));
  HIP_TRY(ctx, md::to_device(d_len, len, n, st));
  HIP_TRY(ctx, md::to_device(d_dst_off, dst_off, n, st));
  HIP_TRY(ctx, md::to_device(d_ids, h_ids, st));
  HIP_TRY(ctx, md::zero(d_rstatus, n, st));
  uint8_t *d_in = ctx->scratch[kBgrIn].as<uint8_t>(), *d_slots = ctx->scratch[kBgrSlots].as<uint8_t>(), *d_dst = ctx->scratch[kHostOut].as<uint8_t>();
  // -- the rounds, one behind the other on the context's stream: nothing comes back in between
  for (const RoundPlan &r : rounds) {
    const size_t t0 = r.t0, count = r.t1 - r.t0;
    for (size_t t = r.t0; t < r.t1;) {  // a run of consecutive members is one piece of src, and of the blob
      size_t e = t + 1;
      while (e < r.t1 && touched[e] == touched[e - 1] + 1) e++;
      const uint64_t b0 = c_off[touched[t]], b1 = c_off[touched[e - 1] + 1];
      HIP_TRY(ctx, md::to_device(d_in + h_mpos[t], src + b0, b1 - b0, st));
      t = e;
    }
    MD_LAUNCH_TRY(ctx, md_launch_gzm_headers(count, d_in, d_mpos + t0, d_mlen + t0, d_body_off + t0, d_body_len + t0, d_isize + t0, d_hstatus + t0, st));
    rc = md_inflate_batch_device(ctx, MD_FORMAT_DEFLATE, count, d_in, d_body_off + t0, d_body_len + t0, d_slots, d_slot + t0, d_cap + t0,
                                 d_out_len + t0, d_consumed + t0, d_status + t0, nullptr);
    if (rc != MD_OK) return rc;
    // (md_launch_gz_finish replaces the decoder's status and count by the member's: the verdict wants both)
    HIP_TRY(ctx, hipMemcpyAsync(d_inf_consumed + t0, d_consumed + t0, count * sizeof *d_consumed, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_inf_status + t0, d_status + t0, count * sizeof *d_status, hipMemcpyDeviceToDevice, st));
    MD_LAUNCH_TRY(ctx, md_launch_gz_finish((uint32_t)count, d_in, d_mpos + t0, d_mlen + t0, d_body_off + t0, d_hstatus + t0, d_slots, d_slot + t0,
                                           d_out_len + t0, d_consumed + t0, d_status + t0, nullptr, st));
    const md::bgr::Round dr{d_mpos + t0,     d_mlen + t0,         d_slot + t0,    d_cap + t0,        d_u0 + t0,     d_body_len + t0,
                            d_isize + t0,    d_inf_consumed + t0, d_hstatus + t0, d_inf_status + t0, d_status + t0, d_verdict + t0};
    MD_LAUNCH_TRY(ctx, md_launch_bgr_verdict((uint32_t)count, d_in, &dr, st));
    MD_LAUNCH_TRY(ctx, md_launch_bgr_gather((uint32_t)count, &dr, (uint32_t)(r.id1 - r.id0), d_ids + r.id0, r.longest, d_off, d_len, d_slots, d_dst,
                                            d_dst_off, d_rstatus, st));
    stats.members += count;
    stats.launches += 1;
    stats.bytes_in += r.in_bytes;
    stats.bytes_scratch += r.slot_bytes;
  }
  // -- the statuses first: a range that failed is not copied out; what is adjacent in dst leaves by one copy
  std::vector<int32_t> got(n);
  HIP_TRY(ctx, md::to_host(got.data(), d_rstatus, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (size_t i = 0; i < n; i++)
    if (status[i] == MD_OK) status[i] = got[i];
  rc = md::adjacent_runs(n, status, len, dst_off, [&](size_t i, uint64_t bytes) -> int {
    HIP_TRY(ctx, md::to_host(dst + dst_off[i], d_dst + dst_off[i], bytes, st));
    return MD_OK;
  });
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return MD_OK;
}

// the checks both reads share; where = off or voff
static int bgzf_read_checks(md_ctx *ctx, const md_bgzf_index *idx, const uint8_t *src, size_t src_len, size_t n, const void *where,
                            const uint64_t *len, const uint64_t *dst_off, const int32_t *status) {
  if (!idx || (!src && src_len) || (n && (!where || !len || !dst_off || !status))) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_bgzf_read: null pointer");
  if (n > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many ranges in one call");
  if (src_len != idx->src_len) return fail(ctx, MD_INVALID_INDEX, "md_bgzf_read: the index belongs to a src of another length");
  return MD_OK;
}

static int bgzf_read_checked(md_ctx *ctx, const md_bgzf_index *idx, const uint8_t *src, size_t n, const uint64_t *off, const uint64_t *len,
                             uint8_t *dst, const uint64_t *dst_off, int32_t *status) {
  const uint64_t size = idx->size();
  bool bytes = false;
  for (size_t i = 0; i < n; i++) {
    if (status[i] != MD_OK) continue;
    if (off[i] > size || len[i] > size - off[i]) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_bgzf_read: a range ends behind the output");
    if (len[i] && dst_off[i] + len[i] < len[i]) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_bgzf_read: a range ends behind the address space");
    bytes = bytes || len[i];
  }
  if (bytes && !dst) return fail(ctx, MD_E_INVALID_ARGUMENT, "md_bgzf_read: null pointer");
  ctx->bgr_last = {};
  if (!bytes) return MD_OK;
  return no_bad_alloc(ctx, "md_bgzf_read", [&] { return bgzf_read_ranges(ctx, idx, src, n, off, len, dst, dst_off, status); });
}

int md_bgzf_read(md_ctx *ctx, const md_bgzf_index *idx, const uint8_t *src, size_t src_len, size_t n, const uint64_t *off, const uint64_t *len,
                 uint8_t *dst, const uint64_t *dst_off, int32_t *status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  const int rc = bgzf_read_checks(ctx, idx, src, src_len, n, off, len, dst_off, status);
  if (rc != MD_OK) return rc;
  for (size_t i = 0; i < n; i++) status[i] = MD_OK;
  return bgzf_read_checked(ctx, idx, src, n, off, len, dst, dst_off, status);
}

int md_bgzf_read_virtual(md_ctx *ctx, const md_bgzf_index *idx, const uint8_t *src, size_t src_len, size_t n, const uint64_t *voff,
                         const uint64_t *len, uint8_t *dst, const uint64_t *dst_off, int32_t *status) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  const int rc = bgzf_read_checks(ctx, idx, src, src_len, n, voff, len, dst_off, status);
  if (rc != MD_OK) return rc;
  return no_bad_alloc(ctx, "md_bgzf_read_virtual", [&] {
    // voff = the member's offset in src << 16 | an offset in its output: the member by binary search over c_off
    std::vector<uint64_t> off(n, 0);
    const size_t M = idx->members();
    for (size_t i = 0; i < n; i++) {
      const uint64_t c = voff[i] >> 16, in = voff[i] & 0xffff;
      const size_t k = (size_t)(std::lower_bound(idx->c_off.begin(), idx->c_off.begin() + M, c) - idx->c_off.begin());
      const bool known = k < M && idx->c_off[k] == c && in <= idx->u_off[k + 1] - idx->u_off[k];
      status[i] = known ? MD_OK : MD_INVALID_INDEX;
      if (known) off[i] = idx->u_off[k] + in;
    }
    return bgzf_read_checked(ctx, idx, src, n, off.data(), len, dst, dst_off, status);
  });
}
