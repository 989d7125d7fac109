// capi_gz_members.cpp — a GZip file of many members (mdeflate.h: md_gz_members_*, md_bgzf_*).
#include <string.h>

#include "ctx.hpp"
#include "gz_rfc.hpp"

// RFC 1952 as libz reads it (gz_rfc.hpp), not Gz.Inf's reading.  The internals work on device pointers; the entry
// points are copy-in, kernels, copy-out.
namespace {
// the members of an indexed file: device arrays of M entries (out_off: M + 1), carved from ctx->scratch[kGzmDesc].p
struct GzmIndex {
  uint64_t M = 0, total = 0;  // members, the sum of their ISIZE fields
  uint64_t *mpos = nullptr, *mlen = nullptr, *body_off = nullptr, *body_len = nullptr, *isize = nullptr, *out_len = nullptr,
           *consumed = nullptr, *out_off = nullptr, *first = nullptr;
  int32_t *hstatus = nullptr, *status = nullptr;
};
}  // namespace

#define MD_LAUNCH_TRY(ctx, expr)                                        \
  do {                                                                  \
    const int e_ = (expr);                                              \
    if (e_ != 0) return fail(ctx, MD_E_HIP, #expr, (hipError_t)e_);     \
  } while (0)

// Mark, chain and descriptors (gz_members.hip) for len bytes at d_src.  *indexed: the chain of BC size fields leads from
// offset 0 to the end of the file; then ix holds the members, their headers parsed and their output offsets scanned.
// Three small read-backs: the candidate count, the member count with the chain's verdict, the total size.
static int gzm_index(md_ctx *ctx, const uint8_t *d_src, uint64_t len, bool *indexed, GzmIndex *ix) {
  *indexed = false;
  if (len < 28) return MD_OK;  // (shorter than any indexed member)
  hipStream_t st = ctx->stream;
  const uint64_t nspans = (len + md::gzm::kMarkSpanBytes - 1) / md::gzm::kMarkSpanBytes, nwords = (len + 31) / 32;
  const size_t words_bytes = (size_t)((nwords + nspans + 1) / 2 * 8);  // bitmap and counts, rounded to 8
  int rc = ctx->scratch[kGzmWs].reserve(ctx, words_bytes + (nspans + 2) * 8, "hipMalloc(member scan)");
  if (rc != MD_OK) return rc;
  uint32_t *bits = (uint32_t *)ctx->scratch[kGzmWs].p, *cnt = bits + nwords;
  uint64_t *base = (uint64_t *)((uint8_t *)ctx->scratch[kGzmWs].p + words_bytes), *last_nz = base + nspans + 1;
  MD_LAUNCH_TRY(ctx, md_launch_gzm_mark(d_src, len, bits, cnt, last_nz, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan32(cnt, nspans, base, st));
  uint64_t C = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&C, base + nspans, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (C == 0 || C > 0x7ffffff0ull) return MD_OK;
  rc = ctx->scratch[kGzmCand].reserve(ctx, (size_t)((3 * C + 1) * 8 + 3 * (C + 2) * 4), "hipMalloc(member candidates)");
  if (rc != MD_OK) return rc;
  uint64_t *cpos = (uint64_t *)ctx->scratch[kGzmCand].p, *cnext = cpos + C, *ridx = cnext + C;
  uint32_t *jump_a = (uint32_t *)(ridx + C + 1), *jump_b = jump_a + C + 2, *reach = jump_b + C + 2;
  MD_LAUNCH_TRY(ctx, md_launch_gzm_compact(d_src, len, bits, base, cpos, cnext, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_chain(C, cpos, cnext, last_nz, jump_a, jump_b, reach, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan32(reach, C, ridx, st));
  uint64_t M = 0;
  uint32_t at_end = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&M, ridx + C, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&at_end, reach + C, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (!at_end || M == 0) return MD_OK;
  rc = ctx->scratch[kGzmDesc].reserve(ctx, (size_t)((8 * M + 2) * 8 + 2 * M * 4), "hipMalloc(member descriptors)");
  if (rc != MD_OK) return rc;
  ix->M = M;
  ix->mpos = (uint64_t *)ctx->scratch[kGzmDesc].p;
  ix->mlen = ix->mpos + M;
  ix->body_off = ix->mlen + M;
  ix->body_len = ix->body_off + M;
  ix->isize = ix->body_len + M;
  ix->out_len = ix->isize + M;
  ix->consumed = ix->out_len + M;
  ix->out_off = ix->consumed + M;  // M + 1
  ix->first = ix->out_off + M + 1;
  ix->hstatus = (int32_t *)(ix->first + 1);
  ix->status = ix->hstatus + M;
  MD_LAUNCH_TRY(ctx, md_launch_gzm_select(C, reach, ridx, cpos, cnext, ix->mpos, ix->mlen, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_headers(M, d_src, ix->mpos, ix->mlen, ix->body_off, ix->body_len, ix->isize, ix->hstatus, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan64(ix->isize, M, ix->out_off, st));
  HIP_TRY(ctx, hipMemcpyAsync(&ix->total, ix->out_off + M, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  *indexed = true;
  return MD_OK;
}

static int gzm_upload(md_ctx *ctx, const uint8_t *src, size_t len) {
  const int rc = ctx->scratch[kHostIn].reserve(ctx, len + 64, "hipMalloc(host path input)");
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch[kHostIn].p, src, len, hipMemcpyHostToDevice, ctx->stream));
  return MD_OK;
}

int md_gz_members_scan(md_ctx *ctx, const uint8_t *src, size_t src_len, md_gz_members_info *info, uint64_t *c_off, uint64_t *u_off,
                       size_t cap) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!info || (!src && src_len) || (cap && (!c_off || !u_off))) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  memset(info, 0, sizeof *info);
  if (src_len == 0) return MD_OK;
  MD_ON_DEVICE(ctx);
  int rc = gzm_upload(ctx, src, src_len);
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
    HIP_TRY(ctx, hipMemcpyAsync(c_off, ix.mpos, k * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(u_off, ix.out_off, k * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
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
    uint64_t hdr = 0;
    st = md::gz::rfc_header(src + pos, len - pos, &hdr);
    if (st != MD_OK) break;
    const size_t body = pos + (size_t)hdr, rest = len - body < MD_MAX_INFLATE_IN ? len - body : (size_t)MD_MAX_INFLATE_IN;
    // where the member ends is the decoder's to say: it gets a window of the file that grows while it runs out of input
    // (a file of many small members is not copied to the device once per member)
    size_t used = 0, wrote = 0;
    for (size_t win = (size_t)256 << 10;; win *= 4) {
      const size_t in = rest < win ? rest : win;
      st = md_de_inf_ns_inflate(ctx, src + body, in, dst ? dst + written : dst, cap - written, &used, &wrote);
      if (st != MD_UNEXPECTED_END_OF_INPUT || in == rest) break;
    }
    if (st < 0) return st;  // (the library's own errors)
    if (st != MD_OK) break;
    if (len - body - used < 8) {
      st = MD_UNEXPECTED_END_OF_INPUT;
      break;
    }
    const uint8_t *t = src + body + used;
    uint32_t want = 0, isize = 0;
    for (int k = 0; k < 4; k++) {
      want |= (uint32_t)t[k] << (8 * k);
      isize |= (uint32_t)t[4 + k] << (8 * k);
    }
    if (want != md::crc32_update(0, dst + written, wrote)) st = MD_INVALID_CHECKSUM;
    else if (isize != (uint32_t)wrote) st = MD_INVALID_SIZE;
    if (st != MD_OK) break;
    pos = body + used + 8;
    written += wrote;
    members++;
  }
  info->members = members;
  info->consumed = pos;
  info->written = written;
  return st;
}

int md_gz_members_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, md_gz_members_info *info) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!info || (!src && src_len) || (!dst && dst_cap)) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  memset(info, 0, sizeof *info);
  if (src_len == 0) return MD_OK;
  MD_ON_DEVICE(ctx);
  int rc = gzm_upload(ctx, src, src_len);
  if (rc != MD_OK) return rc;
  const uint8_t *d_src = (const uint8_t *)ctx->scratch[kHostIn].p;
  bool indexed = false;
  GzmIndex ix;
  rc = gzm_index(ctx, d_src, src_len, &indexed, &ix);
  if (rc != MD_OK) return rc;
  if (!indexed) return gzm_general(ctx, src, src_len, dst, dst_cap, 0, 0, 0, info);
  info->indexed = 1;
  if (ix.total > dst_cap) {
    // The sizes the members state do not fit.  They may lie (a damaged ISIZE), so the host loop decides: it fails where a
    // member really does not fit, or at the member that is wrong - and only in the first case is the answer "more room".
    rc = gzm_general(ctx, src, src_len, dst, dst_cap, 0, 0, 0, info);
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
  HIP_TRY(ctx, hipMemcpyAsync(ix.first, &first, 8, hipMemcpyHostToDevice, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_verdict(ix.M, ix.mlen, ix.consumed, ix.status, ix.first, st));
  HIP_TRY(ctx, hipMemcpyAsync(&first, ix.first, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (first == ix.M) {
    if (ix.total) HIP_TRY(ctx, hipMemcpy(dst, d_out, (size_t)ix.total, hipMemcpyDeviceToHost));
    info->members = (size_t)ix.M;
    info->consumed = src_len;
    info->written = (size_t)ix.total;
    return MD_OK;
  }
  // a member failed: the members in front of it are good and go out; from the failing one on the host loop speaks, so the
  // status is the one the same bytes get without a size index
  uint64_t at[2] = {0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(&at[0], ix.mpos + first, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&at[1], ix.out_off + first, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (at[1]) HIP_TRY(ctx, hipMemcpy(dst, d_out, (size_t)at[1], hipMemcpyDeviceToHost));
  return gzm_general(ctx, src, src_len, dst, dst_cap, (size_t)at[0], (size_t)at[1], (size_t)first, info);
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
  int rc = gzm_upload(ctx, src, src_len);
  if (rc == MD_OK) rc = ctx->scratch[kHostOut].reserve(ctx, nb * stride + 64, "hipMalloc(host path output)");
  if (rc == MD_OK) rc = ctx->scratch[kGzmOut].reserve(ctx, bound + 64, "hipMalloc(blocked gzip file)");
  if (rc == MD_OK) rc = ctx->scratch[kGzmDesc].reserve(ctx, (7 * nb + 2) * 8 + (2 * nb + 2) * 4, "hipMalloc(member descriptors)");
  if (rc != MD_OK) return rc;
  const uint8_t *d_in = (const uint8_t *)ctx->scratch[kHostIn].p;
  uint8_t *slots = (uint8_t *)ctx->scratch[kHostOut].p, *d_file = (uint8_t *)ctx->scratch[kGzmOut].p;
  uint64_t *in_off = (uint64_t *)ctx->scratch[kGzmDesc].p, *in_len = in_off + nb, *out_off = in_len + nb, *out_cap = out_off + nb, *out_len = out_cap + nb,
           *msize = out_len + nb, *moff = msize + nb;  // moff: nb + 1
  int32_t *status = (int32_t *)(moff + nb + 1), *err = status + nb;
  uint32_t *crc = (uint32_t *)(err + 1);
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemsetAsync(err, 0, 4, st));
  if (nb) {
    MD_LAUNCH_TRY(ctx, md_launch_bgzf_plan(nb, src_len, block, stride, in_off, in_len, out_off, out_cap, st));
    // the parameters of MD_FORMAT_GZIP (Gz.Def's make_block: Zl driver, dynamic blocks, queue 4096), the raw body alone
    md_deflate_params p;
    memset(&p, 0, sizeof p);
    p.level = level;
    p.queue_len = 4096;
    p.driver = MD_DRIVER_ZL;
    p.dynamic = 1;
    p.matcher = MD_MATCHER_DE;
    p.total_in_bytes = src_len;
    rc = md_deflate_batch_device(ctx, MD_FORMAT_DEFLATE, &p, nb, d_in, in_off, in_len, slots, out_off, out_cap, out_len, status, nullptr);
    if (rc != MD_OK) return rc;
    MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)nb, d_in, in_off, in_len, crc, st));
    MD_LAUNCH_TRY(ctx, md_launch_bgzf_sizes(nb, in_len, out_len, status, msize, err, st));
  }
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan64(msize, nb, moff, st));
  MD_LAUNCH_TRY(ctx, md_launch_bgzf_pack(nb, d_in, in_off, in_len, slots, out_off, out_len, status, moff, crc, d_file, st));
  uint64_t total = 0;
  int32_t bad = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&total, moff + nb, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&bad, err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (bad != 0) return bad;  // (MD_QUEUE_FULL: not with this queue, said all the same)
  if (total + 28 > bound) return fail(ctx, MD_E_HIP, "blocked gzip: member sizes above the bound");
  if (total + 28 > dst_cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  HIP_TRY(ctx, hipMemcpy(dst, d_file, (size_t)total + 28, hipMemcpyDeviceToHost));
  *written = (size_t)total + 28;
  return MD_OK;
}
#undef MD_LAUNCH_TRY
