// capi_gz_members.cpp — a GZip file of many members (mdeflate.h: md_gz_members_*, md_bgzf_*).
#include <string.h>

#include <vector>

#include "ctx.hpp"
#include "gz_rfc.hpp"

// RFC 1952 as libz reads it (gz_rfc.hpp), not Gz.Inf's reading.  The internals work on device pointers; the entry
// points are copy-in, kernels, copy-out.

// Mark, chain and descriptors (gz_members.hip) for len bytes at d_src.  *indexed: the chain of BC size fields leads from
// offset 0 to the end of the file; then ix holds the members, their headers parsed and their output offsets scanned.
// Three small read-backs: the candidate count, the member count with the chain's verdict, the total size.
int gzm_index(md_ctx *ctx, const uint8_t *d_src, uint64_t len, bool *indexed, GzmIndex *ix) {
  *indexed = false;
  if (len < 28) return MD_OK;  // (shorter than any indexed member)
  hipStream_t st = ctx->stream;
  const uint64_t nspans = (len + md::gzm::kMarkSpanBytes - 1) / md::gzm::kMarkSpanBytes, nwords = (len + 31) / 32;
  uint32_t *bits = nullptr, *cnt = nullptr;  // the bitmap of marks, the marks per span
  uint64_t *base = nullptr, *last_nz = nullptr;
  int rc = carve(ctx, ctx->scratch[kGzmWs], "hipMalloc(member scan)", [&](md::Carver &ws) {
    bits = ws.take<uint32_t>(nwords), cnt = ws.take<uint32_t>(nspans);
    base = ws.take<uint64_t>(nspans + 1), last_nz = ws.take<uint64_t>(1);
  });
  if (rc != MD_OK) return rc;
  MD_LAUNCH_TRY(ctx, md_launch_gzm_mark(d_src, len, bits, cnt, last_nz, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan32(cnt, nspans, base, st));
  uint64_t C = 0;
  HIP_TRY(ctx, md::to_host(&C, base + nspans, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (C == 0 || C > 0x7ffffff0ull) return MD_OK;
  uint64_t *cpos = nullptr, *cnext = nullptr, *ridx = nullptr;
  uint32_t *jump_a = nullptr, *jump_b = nullptr, *reach = nullptr;
  rc = carve(ctx, ctx->scratch[kGzmCand], "hipMalloc(member candidates)", [&](md::Carver &cand) {
    cpos = cand.take<uint64_t>(C), cnext = cand.take<uint64_t>(C), ridx = cand.take<uint64_t>(C + 1);
    jump_a = cand.take<uint32_t>(C + 2), jump_b = cand.take<uint32_t>(C + 2), reach = cand.take<uint32_t>(C + 2);
  });
  if (rc != MD_OK) return rc;
  MD_LAUNCH_TRY(ctx, md_launch_gzm_compact(d_src, len, bits, base, cpos, cnext, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_chain(C, cpos, cnext, last_nz, jump_a, jump_b, reach, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan32(reach, C, ridx, st));
  uint64_t M = 0;
  uint32_t at_end = 0;
  HIP_TRY(ctx, md::to_host(&M, ridx + C, 1, st));
  HIP_TRY(ctx, md::to_host(&at_end, reach + C, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (!at_end || M == 0) return MD_OK;
  ix->M = M;
  rc = carve(ctx, ctx->scratch[kGzmDesc], "hipMalloc(member descriptors)", [&](md::Carver &desc) {
    ix->mpos = desc.take<uint64_t>(M), ix->mlen = desc.take<uint64_t>(M), ix->body_off = desc.take<uint64_t>(M), ix->body_len = desc.take<uint64_t>(M);
    ix->isize = desc.take<uint64_t>(M), ix->out_len = desc.take<uint64_t>(M), ix->consumed = desc.take<uint64_t>(M);
    ix->out_off = desc.take<uint64_t>(M + 1), ix->first = desc.take<uint64_t>(1);
    ix->hstatus = desc.take<int32_t>(M), ix->status = desc.take<int32_t>(M);
  });
  if (rc != MD_OK) return rc;
  MD_LAUNCH_TRY(ctx, md_launch_gzm_select(C, reach, ridx, cpos, cnext, ix->mpos, ix->mlen, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_headers(M, d_src, ix->mpos, ix->mlen, ix->body_off, ix->body_len, ix->isize, ix->hstatus, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan64(ix->isize, M, ix->out_off, st));
  HIP_TRY(ctx, md::to_host(&ix->total, ix->out_off + M, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  *indexed = true;
  return MD_OK;
}

int md_gz_members_scan(md_ctx *ctx, const uint8_t *src, size_t src_len, md_gz_members_info *info, uint64_t *c_off, uint64_t *u_off,
                       size_t cap) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!info || (!src && src_len) || (cap && (!c_off || !u_off))) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  memset(info, 0, sizeof *info);
  if (src_len == 0) return MD_OK;
  MD_ON_DEVICE(ctx);
  int rc = upload_host_in(ctx, src, src_len);
  if (rc != MD_OK) return rc;
  bool indexed = false;
  GzmIndex ix;
  rc = gzm_index(ctx, (const uint8_t *)ctx->scratch[kHostIn].p, src_len, &indexed, &ix);
  if (rc != MD_OK || !indexed) return rc;
  info->indexed = 1;
  info->members = (size_t)ix.M;
  info->consumed = src_len;
  info->written = (size_t)ix.total;
  const size_t k = cap < ix.M ? cap : (size_t)ix.M;
  if (k) {
    HIP_TRY(ctx, md::to_host(c_off, ix.mpos, k, ctx->stream));
    HIP_TRY(ctx, md::to_host(u_off, ix.out_off, k, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MD_OK;
}

// One member at *pos, as libz reads it: header on the host, the body through md_de_inf_ns_inflate straight into dst behind
// the *written bytes it holds, CRC-32 and ISIZE.  MD_OK: *pos is the byte behind its trailer and *written counts its
// bytes.  Anything else (negative: the library's own errors) leaves both alone.
static int gzm_member(md_ctx *ctx, const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t *pos, size_t *written) {
  uint64_t hdr = 0;
  int st = md::gz::rfc_header(src + *pos, len - *pos, &hdr);
  if (st != MD_OK) return st;
  const size_t body = *pos + (size_t)hdr, rest = len - body < MD_MAX_INFLATE_IN ? len - body : (size_t)MD_MAX_INFLATE_IN;
  // where the member ends is the decoder's to say: it gets a window of the file that grows while it runs out of input
  // (a file of many small members is not copied to the device once per member)
  size_t used = 0, wrote = 0;
  for (size_t win = (size_t)256 << 10;; win *= 4) {
    const size_t in = rest < win ? rest : win;
    st = md_de_inf_ns_inflate(ctx, src + body, in, dst ? dst + *written : dst, cap - *written, &used, &wrote);
    if (st != MD_UNEXPECTED_END_OF_INPUT || in == rest) break;
  }
  if (st != MD_OK) return st;
  if (len - body - used < 8) return MD_UNEXPECTED_END_OF_INPUT;
  const uint8_t *t = src + body + used;
  if (md::le32(t) != md::crc32_update(0, dst + *written, wrote)) return MD_INVALID_CHECKSUM;
  if (md::le32(t + 4) != (uint32_t)wrote) return MD_INVALID_SIZE;
  *pos = body + used + 8;
  *written += wrote;
  return MD_OK;
}

// The general path: member by member from offset `pos` on, `written` bytes and `members` members already in dst.
static int gzm_general(md_ctx *ctx, const uint8_t *src, size_t len, uint8_t *dst, size_t cap, size_t pos, size_t written, size_t members,
                       md_gz_members_info *info) {
  int st = MD_OK;
  for (;;) {
    if (members) {  // NUL bytes behind a member are padding (gzip(1), libz's gzread and Python skip them)
      while (pos < len && src[pos] == 0) pos++;
    }
    if (pos == len) break;
    st = gzm_member(ctx, src, len, dst, cap, &pos, &written);
    if (st < 0) return st;  // (the library's own errors)
    if (st != MD_OK) break;
    members++;
  }
  info->members = members;
  info->consumed = pos;
  info->written = written;
  return st;
}

// ---- a file that does not state its members' lengths: speculation and verification (gz_spec.hip) ----
namespace {
constexpr uint64_t kSpecMinCandidates = 2;  // fewer: one member (or none that starts at offset 0), the host loop's case
// what the walk needs of the batch: per candidate its position, the size it promised if the batch let it in, and its flag
struct SpecBatch {
  std::vector<uint64_t> cpos, pass;
  std::vector<uint8_t> flag;
  const uint8_t *d_out = nullptr;  // the batch's output: span k's bytes at the sum of pass[0 .. k)
};
}  // namespace

// (no error text: whatever fails here, the caller clears HIP's error and the host loop reads the file)
#define SPEC_TRY(expr)                        \
  do {                                        \
    if ((int)(expr) != 0) return MD_E_HIP;    \
  } while (0)

// Mark, compact, spans, classify, the inflate launch over every admitted span, gz_finish, verify.  MD_NOT_HANDLED: fewer
// than two candidates or none at offset 0.  Three read-backs: the candidate count, the sum of the admitted guesses (it
// sizes the output), the candidates' 17 bytes each.
static int gzm_spec_batch(md_ctx *ctx, const uint8_t *d_src, uint64_t len, uint64_t dst_cap, SpecBatch *b) {
  hipStream_t st = ctx->stream;
  const uint64_t nspans = (len + md::gzm::kMarkSpanBytes - 1) / md::gzm::kMarkSpanBytes, nwords = (len + 31) / 32;
  uint32_t *bits = nullptr, *cnt = nullptr;  // (as gzm_index)
  uint64_t *base = nullptr;
  int rc = carve(ctx, ctx->scratch[kGzmWs], nullptr, [&](md::Carver &ws) {
    bits = ws.take<uint32_t>(nwords), cnt = ws.take<uint32_t>(nspans);
    base = ws.take<uint64_t>(nspans + 1);
  });
  if (rc != MD_OK) return rc;
  SPEC_TRY(md_launch_gzs_mark(d_src, len, bits, cnt, st));
  SPEC_TRY(md_launch_gzm_scan32(cnt, nspans, base, st));
  uint64_t C = 0;
  uint32_t word0 = 0;
  SPEC_TRY(md::to_host(&C, base + nspans, 1, st));
  SPEC_TRY(md::to_host(&word0, bits, 1, st));
  SPEC_TRY(hipStreamSynchronize(st));
  if (C < kSpecMinCandidates || !(word0 & 1) || C > 0x7ffffff0ull) return MD_NOT_HANDLED;
  rc = ctx->scratch[kGzmCand].reserve(ctx, (size_t)C * sizeof(uint64_t), nullptr);
  if (rc != MD_OK) return rc;
  uint64_t *cpos = ctx->scratch[kGzmCand].as<uint64_t>();
  uint64_t *mlen = nullptr, *body_off = nullptr, *body_len = nullptr, *guess = nullptr, *pass = nullptr, *dec_len = nullptr, *out_cap = nullptr,
           *out_len = nullptr, *consumed = nullptr, *out_off = nullptr;
  int32_t *hstatus = nullptr, *status = nullptr;
  uint8_t *flag = nullptr;
  rc = carve(ctx, ctx->scratch[kGzmDesc], nullptr, [&](md::Carver &desc) {
    mlen = desc.take<uint64_t>(C), body_off = desc.take<uint64_t>(C), body_len = desc.take<uint64_t>(C), guess = desc.take<uint64_t>(C);
    pass = desc.take<uint64_t>(C), dec_len = desc.take<uint64_t>(C), out_cap = desc.take<uint64_t>(C), out_len = desc.take<uint64_t>(C);
    consumed = desc.take<uint64_t>(C), out_off = desc.take<uint64_t>(C + 1);
    hstatus = desc.take<int32_t>(C), status = desc.take<int32_t>(C);
    flag = desc.take<uint8_t>(C);
  });
  if (rc != MD_OK) return rc;
  SPEC_TRY(md_launch_gzs_compact(len, bits, base, cpos, st));
  SPEC_TRY(md_launch_gzs_spans(C, cpos, len, mlen, st));
  SPEC_TRY(md_launch_gzm_headers(C, d_src, cpos, mlen, body_off, body_len, guess, hstatus, st));
  SPEC_TRY(md_launch_gzm_scan64(body_len, C, out_off, st));  // (out_off[C]: the sum of all bodies, for rule (c))
  SPEC_TRY(md_launch_gzs_classify(C, hstatus, body_len, guess, out_off + C, ctx->par_min, pass, flag, st));
  SPEC_TRY(md_launch_gzm_scan64(pass, C, out_off, st));
  uint64_t total = 0;
  SPEC_TRY(md::to_host(&total, out_off + C, 1, st));
  SPEC_TRY(md_launch_gzs_room(C, body_len, pass, dst_cap, out_off, dec_len, out_cap, flag, st));
  SPEC_TRY(hipStreamSynchronize(st));
  // no admitted span ends behind dst_cap (rule (d)), and none behind the sum
  rc = ctx->scratch[kGzmOut].reserve(ctx, (size_t)(total < dst_cap ? total : dst_cap) + 64, nullptr);
  if (rc != MD_OK) return rc;
  uint8_t *d_out = (uint8_t *)ctx->scratch[kGzmOut].p;
  rc = md_inflate_batch_device(ctx, MD_FORMAT_DEFLATE, (size_t)C, d_src, body_off, dec_len, d_out, out_off, out_cap, out_len, consumed, status, nullptr);
  if (rc != MD_OK) return rc;
  SPEC_TRY(md_launch_gz_finish((uint32_t)C, d_src, cpos, mlen, body_off, hstatus, d_out, out_off, out_len, consumed, status, nullptr, st));
  SPEC_TRY(md_launch_gzs_verify(C, mlen, hstatus, status, consumed, out_len, pass, flag, st));
  b->cpos.resize((size_t)C);
  b->pass.resize((size_t)C);
  b->flag.resize((size_t)C);
  SPEC_TRY(md::to_host(b->cpos.data(), cpos, (size_t)C, st));
  SPEC_TRY(md::to_host(b->pass.data(), pass, (size_t)C, st));
  SPEC_TRY(md::to_host(b->flag.data(), flag, (size_t)C, st));
  SPEC_TRY(hipStreamSynchronize(st));
  b->d_out = d_out;
  return MD_OK;
}

// The file as libz reads it, from offset 0: a member whose start is a verified span comes from the batch, any other is one
// step of the host loop.  MD_NOT_HANDLED: nothing of this path stands (info and dst are the caller's to fill again).
static int gzm_speculative(md_ctx *ctx, const uint8_t *d_src, const uint8_t *src, size_t len, uint8_t *dst, size_t cap, md_gz_members_info *info) {
  SpecBatch b;
  int rc = gzm_spec_batch(ctx, d_src, len, cap, &b);
  if (rc != MD_OK) return MD_NOT_HANDLED;
  md_gz_members_stats &stats = ctx->gzm_last;
  const size_t C = b.cpos.size();
  stats.path = 2;
  stats.candidates = C;
  for (size_t k = 0; k < C; k++) {
    const uint32_t why = b.flag[k] >> 1;
    stats.spans_decoded += why == md::gzs::kSpanAdmitted;
    stats.spans_implausible += why == md::gzs::kSpanImplausible;
    stats.spans_long += why == md::gzs::kSpanLong;
    stats.spans_no_room += why == md::gzs::kSpanNoRoom;
  }
  size_t pos = 0, written = 0, members = 0, k = 0;
  uint64_t off = 0;                 // where span k's bytes begin in the batch's output: the sum of pass[0 .. k)
  size_t run_off = 0, run_len = 0;  // accepted members not yet in dst: consecutive spans, so one piece of the batch's output
  const auto flush = [&]() {
    const bool ok = run_len == 0 || hipMemcpy(dst + written - run_len, b.d_out + run_off, run_len, hipMemcpyDeviceToHost) == hipSuccess;
    run_len = 0;
    return ok;
  };
  int st = MD_OK;
  for (;;) {
    if (members) {  // (as gzm_general)
      while (pos < len && src[pos] == 0) pos++;
    }
    if (pos == len) break;
    while (k < C && b.cpos[k] < pos) off += b.pass[k++];
    if (k < C && b.cpos[k] == pos && (b.flag[k] & md::gzs::kSpanVerified)) {
      const size_t size = (size_t)b.pass[k];
      if (size > cap - written) {  // (what the decoder of the host step says of a valid member without room)
        st = MD_UNEXPECTED_END_OF_OUTPUT;
        break;
      }
      if (run_len == 0) run_off = (size_t)off;
      run_len += size;
      written += size;
      members++;
      stats.members_device++;
      pos = k + 1 < C ? (size_t)b.cpos[k + 1] : len;
      continue;
    }
    if (!flush()) return MD_NOT_HANDLED;
    st = gzm_member(ctx, src, len, dst, cap, &pos, &written);
    if (st < 0) return st;
    if (st != MD_OK) break;
    members++;
    stats.members_host++;
  }
  if (!flush()) return MD_NOT_HANDLED;
  info->members = members;
  info->consumed = pos;
  info->written = written;
  return st;
}
#undef SPEC_TRY

int md_gz_members_last(const md_ctx *ctx, md_gz_members_stats *out) {
  if (!ctx || !out) return MD_E_INVALID_ARGUMENT;
  *out = ctx->gzm_last;
  return MD_OK;
}

int md_gz_members_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, md_gz_members_info *info) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!info || (!src && src_len) || (!dst && dst_cap)) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  memset(info, 0, sizeof *info);
  md_gz_members_stats &stats = ctx->gzm_last;
  stats = md_gz_members_stats{};
  if (src_len == 0) return MD_OK;
  MD_ON_DEVICE(ctx);
  int rc = upload_host_in(ctx, src, src_len);
  if (rc != MD_OK) return rc;
  const uint8_t *d_src = (const uint8_t *)ctx->scratch[kHostIn].p;
  bool indexed = false;
  GzmIndex ix;
  rc = gzm_index(ctx, d_src, src_len, &indexed, &ix);
  if (rc != MD_OK) return rc;
  if (!indexed) {
    if (ctx->gzm_speculate) {
      rc = gzm_speculative(ctx, d_src, src, src_len, dst, dst_cap, info);
      if (rc != MD_NOT_HANDLED) return rc;
      // an allocation, a launch or a copy failed, or the file is no case for it: a valid file must not fail where the host
      // loop reads it
      (void)hipGetLastError();
      stats = md_gz_members_stats{};
    }
    rc = gzm_general(ctx, src, src_len, dst, dst_cap, 0, 0, 0, info);
    stats.members_host = info->members;
    return rc;
  }
  info->indexed = 1;
  stats.path = 1;
  if (ix.total > dst_cap) {
    // The sizes the members state do not fit.  They may lie (a damaged ISIZE), so the host loop decides: it fails where a
    // member really does not fit, or at the member that is wrong - and only in the first case is the answer "more room".
    rc = gzm_general(ctx, src, src_len, dst, dst_cap, 0, 0, 0, info);
    stats.members_host = info->members;
    if (rc == MD_UNEXPECTED_END_OF_OUTPUT) info->written = (size_t)ix.total;
    return rc;
  }
  // every member at once: the inflate launch over the bodies, each into the ISIZE bytes its trailer promises (a member
  // that lies about its size cannot write into its neighbour), then CRC-32 and ISIZE per member, then the verdict
  rc = ctx->scratch[kHostOut].reserve(ctx, (size_t)ix.total + 64, "hipMalloc(host path output)");
  if (rc != MD_OK) return rc;
  uint8_t *d_out = (uint8_t *)ctx->scratch[kHostOut].p;
  hipStream_t st = ctx->stream;
  rc = md_inflate_batch_device(ctx, MD_FORMAT_DEFLATE, (size_t)ix.M, d_src, ix.body_off, ix.body_len, d_out, ix.out_off, ix.isize, ix.out_len,
                               ix.consumed, ix.status, nullptr);
  if (rc != MD_OK) return rc;
  MD_LAUNCH_TRY(ctx, md_launch_gz_finish((uint32_t)ix.M, d_src, ix.mpos, ix.mlen, ix.body_off, ix.hstatus, d_out, ix.out_off, ix.out_len,
                                         ix.consumed, ix.status, nullptr, st));
  uint64_t first = ix.M;
  HIP_TRY(ctx, md::to_device(ix.first, &first, 1, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_verdict(ix.M, ix.mlen, ix.consumed, ix.status, ix.first, st));
  HIP_TRY(ctx, md::to_host(&first, ix.first, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (first == ix.M) {
    if (ix.total) HIP_TRY(ctx, hipMemcpy(dst, d_out, (size_t)ix.total, hipMemcpyDeviceToHost));
    info->members = (size_t)ix.M;
    info->consumed = src_len;
    info->written = (size_t)ix.total;
    stats.members_device = (size_t)ix.M;
    return MD_OK;
  }
  // a member failed: the members in front of it are good and go out; from the failing one on the host loop speaks, so the
  // status is the one the same bytes get without a size index
  uint64_t at[2] = {0, 0};
  HIP_TRY(ctx, md::to_host(&at[0], ix.mpos + first, 1, st));
  HIP_TRY(ctx, md::to_host(&at[1], ix.out_off + first, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (at[1]) HIP_TRY(ctx, hipMemcpy(dst, d_out, (size_t)at[1], hipMemcpyDeviceToHost));
  rc = gzm_general(ctx, src, src_len, dst, dst_cap, (size_t)at[0], (size_t)at[1], (size_t)first, info);
  stats.members_device = (size_t)first;
  stats.members_host = info->members - (size_t)first;
  return rc;
}

static const size_t kBgzfBlockMax = 0xff00;  // htslib's block: 64 KiB less room for a member that does not compress

size_t md_bgzf_compress_bound(size_t src_len, size_t block) {
  if (block == 0) block = kBgzfBlockMax;
  if (block > kBgzfBlockMax) return 0;
  const size_t nb = src_len / block + (src_len % block ? 1 : 0);
  return src_len + 31 * nb + 28;  // per block 18 + (01 LEN NLEN) + 8, the stored form; the EOF marker
}

int md_bgzf_compress(md_ctx *ctx, int level, size_t block, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                     size_t *written) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!written || (!src && src_len) || (!dst && dst_cap)) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  *written = 0;
  if (block == 0) block = kBgzfBlockMax;
  if (block > kBgzfBlockMax) return fail(ctx, MD_E_INVALID_ARGUMENT, "a BGZF block holds at most 0xff00 bytes");
  if (level < 0 || level > 9) return fail(ctx, MD_E_INVALID_ARGUMENT, "Invalid level of compression");
  const size_t nb = src_len / block + (src_len % block ? 1 : 0);
  if (nb > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many blocks in one call");
  if (dst_cap < 28) return MD_UNEXPECTED_END_OF_OUTPUT;
  MD_ON_DEVICE(ctx);
  // slots of fixed stride for the bodies: a body longer than block + 5 bytes loses against the stored form anyway (the
  // encoder then says MD_UNEXPECTED_END_OF_OUTPUT for that slot, and the pack kernel writes the block stored)
  const size_t stride = (block + 5 + 15) & ~(size_t)15, bound = md_bgzf_compress_bound(src_len, block);
  int rc = upload_host_in(ctx, src, src_len);
  if (rc == MD_OK) rc = ctx->scratch[kHostOut].reserve(ctx, nb * stride + 64, "hipMalloc(host path output)");
  if (rc == MD_OK) rc = ctx->scratch[kGzmOut].reserve(ctx, bound + 64, "hipMalloc(blocked gzip file)");
  if (rc != MD_OK) return rc;
  const uint8_t *d_in = (const uint8_t *)ctx->scratch[kHostIn].p;
  uint8_t *slots = (uint8_t *)ctx->scratch[kHostOut].p, *d_file = (uint8_t *)ctx->scratch[kGzmOut].p;
  uint64_t *in_off = nullptr, *in_len = nullptr, *out_off = nullptr, *out_cap = nullptr, *out_len = nullptr, *msize = nullptr, *moff = nullptr;
  int32_t *status = nullptr, *err = nullptr;
  uint32_t *crc = nullptr;
  rc = carve(ctx, ctx->scratch[kGzmDesc], "hipMalloc(member descriptors)", [&](md::Carver &desc) {
    in_off = desc.take<uint64_t>(nb), in_len = desc.take<uint64_t>(nb), out_off = desc.take<uint64_t>(nb), out_cap = desc.take<uint64_t>(nb);
    out_len = desc.take<uint64_t>(nb), msize = desc.take<uint64_t>(nb), moff = desc.take<uint64_t>(nb + 1);
    status = desc.take<int32_t>(nb), err = desc.take<int32_t>(1);
    crc = desc.take<uint32_t>(nb);
  });
  if (rc != MD_OK) return rc;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, md::zero(err, 1, st));
  if (nb) {
    MD_LAUNCH_TRY(ctx, md_launch_bgzf_plan(nb, src_len, block, stride, in_off, in_len, out_off, out_cap, st));
    const md_deflate_params p = gzip_body_params(level, src_len);
    rc = md_deflate_batch_device(ctx, MD_FORMAT_DEFLATE, &p, nb, d_in, in_off, in_len, slots, out_off, out_cap, out_len, status, nullptr);
    if (rc != MD_OK) return rc;
    MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)nb, d_in, in_off, in_len, crc, st));
    MD_LAUNCH_TRY(ctx, md_launch_bgzf_sizes(nb, in_len, out_len, status, msize, err, st));
  }
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan64(msize, nb, moff, st));
  MD_LAUNCH_TRY(ctx, md_launch_bgzf_pack(nb, d_in, in_off, in_len, slots, out_off, out_len, status, moff, crc, d_file, st));
  uint64_t total = 0;
  int32_t bad = 0;
  HIP_TRY(ctx, md::to_host(&total, moff + nb, 1, st));
  HIP_TRY(ctx, md::to_host(&bad, err, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (bad != 0) return bad;  // (MD_QUEUE_FULL: not with this queue, said all the same)
  if (total + 28 > bound) return fail(ctx, MD_E_HIP, "blocked gzip: member sizes above the bound");
  if (total + 28 > dst_cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  HIP_TRY(ctx, hipMemcpy(dst, d_file, (size_t)total + 28, hipMemcpyDeviceToHost));
  *written = (size_t)total + 28;
  return MD_OK;
}
