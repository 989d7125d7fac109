// capi_zip.cpp — ZIP archives (mdeflate.h: md_zip_directory, md_zip_uncompress, md_zip_compress_bound, md_zip_compress).
// The directory is the host's (zip_dir.hpp); local headers, bodies and checksums are the device's (zip_kernels.hip).
#include <string.h>

#include <new>
#include <vector>

#include "ctx.hpp"
#include "zip_dir.hpp"

namespace {
// The table segment -> entry of entries of len[j] bytes in segments of seg bytes: first[j] = entry j's first segment
// (k + 1 words), seg_entry[s] = the entry of segment s.  An empty entry has no segment.
void segment_table(const std::vector<uint64_t> &len, uint64_t seg, std::vector<uint64_t> *first, std::vector<uint32_t> *seg_entry) {
  const size_t k = len.size();
  first->resize(k + 1);
  uint64_t n = 0;
  for (size_t j = 0; j < k; j++) {
    (*first)[j] = n;
    n += len[j] / seg + (len[j] % seg ? 1 : 0);
  }
  (*first)[k] = n;
  seg_entry->resize((size_t)n);
  for (size_t j = 0; j < k; j++)
    for (uint64_t s = (*first)[j]; s < (*first)[j + 1]; s++) (*seg_entry)[(size_t)s] = (uint32_t)j;
}
}  // namespace

int md_zip_directory(const uint8_t *src, size_t src_len, md_zip_info *info, md_zip_entry *entries, size_t cap) {
  if (!src || !info || (cap && !entries)) return MD_E_INVALID_ARGUMENT;
  return md::zip::read_directory(src, src_len, info, entries, cap);
}

static int zip_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, const uint64_t *select, size_t nselect, uint8_t *dst, size_t dst_cap,
                          uint64_t *out_off, int32_t *status, md_zip_result *res) {
  md_zip_info info;
  int rc = md::zip::read_directory(src, src_len, &info, nullptr, 0);
  if (rc != MD_OK) return rc;
  std::vector<md_zip_entry> dir(info.entries);
  rc = md::zip::read_directory(src, src_len, &info, dir.data(), dir.size());
  if (rc != MD_OK) return rc;
  const size_t k = select ? nselect : info.entries;
  if (k > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many entries in one call");
  if (k && !status) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  for (size_t j = 0; select && j < k; j++)
    if (select[j] >= info.entries) return fail(ctx, MD_E_INVALID_ARGUMENT, "selected entry out of range");
  // the rows, the names and the room: the directory's word alone
  std::vector<md::zip::Row> rows(k);
  std::vector<uint64_t> usize(k);
  std::vector<uint8_t> names;
  const uint64_t dir_at = info.prefix + info.dir_off;  // where the directory begins: no header or body reaches it
  uint64_t lo = dir_at, hi = 0;
  for (size_t j = 0; j < k; j++) {
    const md_zip_entry &e = dir[select ? (size_t)select[j] : j];
    md::zip::Row &r = rows[j];
    memset(&r, 0, sizeof r);
    r.header_off = e.header_off;
    r.csize = e.csize;
    r.usize = usize[j] = e.usize;
    r.name_pos = names.size();
    r.crc = e.crc32;
    r.name_len = e.name_len;
    r.method = e.method;
    r.flags = e.flags;
    names.insert(names.end(), src + e.name_off, src + e.name_off + e.name_len);
    if (e.header_off < dir_at) {
      // the body ends at most 30 + name + 65 535 (the local extra field, unknown here) + csize behind the header
      const uint64_t room = dir_at - e.header_off, frame = 30 + (uint64_t)e.name_len + 0xffff;
      const uint64_t end = e.header_off + (e.csize > room || frame + e.csize > room ? room : frame + e.csize);
      if (e.header_off < lo) lo = e.header_off;
      if (end > hi) hi = end;
    }
  }
  const uint64_t need = md::running_offsets(k, out_off, [&](size_t j) { return usize[j]; });
  res->entries = k;
  res->written = need;
  if (need > dst_cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  if (k == 0) return MD_OK;
  if (hi < lo) hi = lo;
  const uint64_t seg = ctx->zip_segment;
  std::vector<uint64_t> first;
  std::vector<uint32_t> seg_entry;
  segment_table(usize, seg, &first, &seg_entry);
  const size_t nseg = seg_entry.size();

  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  md::zip::Row *d_rows = nullptr;
  uint64_t *d_usize = nullptr, *d_out_off = nullptr, *d_first = nullptr, *in_off = nullptr, *in_len = nullptr, *out_cap = nullptr, *body_off = nullptr,
           *out_len = nullptr, *consumed = nullptr, *failed = nullptr;
  int32_t *hstatus = nullptr, *d_status = nullptr;
  uint32_t *d_seg_entry = nullptr, *crc = nullptr;
  uint8_t *kind = nullptr, *d_names = nullptr;
  rc = carve(ctx, ctx->scratch[kZipDesc], "hipMalloc(zip descriptors)", [&](md::Carver &c) {
    d_rows = c.take<md::zip::Row>(k);
    d_usize = c.take<uint64_t>(k);
    d_out_off = c.take<uint64_t>(k + 1);
    d_first = c.take<uint64_t>(k + 1);
    in_off = c.take<uint64_t>(k);
    in_len = c.take<uint64_t>(k);
    out_cap = c.take<uint64_t>(k);
    body_off = c.take<uint64_t>(k);
    out_len = c.take<uint64_t>(k);
    consumed = c.take<uint64_t>(k);
    failed = c.take<uint64_t>(1);
    hstatus = c.take<int32_t>(k);
    d_status = c.take<int32_t>(k);
    d_seg_entry = c.take<uint32_t>(nseg);
    crc = c.take<uint32_t>(nseg);
    kind = c.take<uint8_t>(k);
    d_names = c.take<uint8_t>(names.size());
  });
  if (rc == MD_OK) rc = upload_host_in(ctx, src + lo, (size_t)(hi - lo));
  if (rc == MD_OK) rc = ctx->scratch[kHostOut].reserve(ctx, (size_t)need + 64, "hipMalloc(host path output)");
  if (rc != MD_OK) return rc;
  uint8_t *d_src = (uint8_t *)ctx->scratch[kHostIn].p, *d_out = (uint8_t *)ctx->scratch[kHostOut].p;
  HIP_TRY(ctx, md::to_device(d_rows, rows, st));
  HIP_TRY(ctx, md::to_device(d_usize, usize, st));
  HIP_TRY(ctx, md::to_device(d_out_off, out_off, k + 1, st));
  HIP_TRY(ctx, md::to_device(d_first, first, st));
  HIP_TRY(ctx, md::to_device(d_seg_entry, seg_entry, st));
  HIP_TRY(ctx, md::to_device(d_names, names, st));
  HIP_TRY(ctx, md::zero(failed, 1, st));
  MD_LAUNCH_TRY(ctx, md_launch_zip_local(k, d_rows, d_src, lo, hi, d_names, in_off, in_len, out_cap, body_off, hstatus, kind, st));
  // every deflated entry at once, each into the usize bytes the directory promises: an entry that lies about its size
  // cannot write into its neighbour (stored entries and those without a good header are streams of no input and no room)
  rc = md_inflate_batch_device(ctx, MD_FORMAT_DEFLATE, k, d_src, in_off, in_len, d_out, d_out_off, out_cap, out_len, consumed, d_status, nullptr);
  if (rc != MD_OK) return rc;
  MD_LAUNCH_TRY(ctx, md_launch_zip_segments(nseg, seg, d_seg_entry, d_first, d_usize, kind, d_src, body_off, d_out, d_out_off, crc, st));
  MD_LAUNCH_TRY(ctx, md_launch_zip_verdict(k, d_rows, d_first, seg, crc, hstatus, out_len, consumed, d_status, failed, st));
  uint64_t nfailed = 0;
  HIP_TRY(ctx, md::to_host(status, d_status, k, st));
  HIP_TRY(ctx, md::to_host(&nfailed, failed, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (need) HIP_TRY(ctx, hipMemcpy(dst, d_out, (size_t)need, hipMemcpyDeviceToHost));
  res->failed = (size_t)nfailed;
  return MD_OK;
}

int md_zip_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, const uint64_t *select, size_t nselect, uint8_t *dst, size_t dst_cap,
                      uint64_t *out_off, int32_t *status, md_zip_result *res) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!src || !res || !out_off || (!dst && dst_cap)) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  memset(res, 0, sizeof *res);
  return no_bad_alloc(ctx, "host memory for the archive's directory",
                      [&] { return zip_uncompress(ctx, src, src_len, select, nselect, dst, dst_cap, out_off, status, res); });
}

// ---- the writer ----
static const uint64_t kZipFileFrame = 76, kZipEndFrame = 98;  // local + central header without the names; 22 + 56 + 20
static const size_t kZip64From = 0xffff;                      // files from which the ZIP64 end record is written

size_t md_zip_compress_bound(size_t n, const md_zip_source *files) {
  if (n && !files) return 0;
  uint64_t sum = kZipEndFrame;
  for (size_t i = 0; i < n; i++) {
    const md_zip_source &f = files[i];
    if (f.name_len == 0 || f.name_len > 0xffff) return 0;
    const uint64_t frame = kZipFileFrame + 2 * (uint64_t)f.name_len;
    if (f.len > UINT64_MAX - frame || sum > UINT64_MAX - frame - f.len) return 0;
    sum += frame + f.len;
  }
  return sum > SIZE_MAX ? 0 : (size_t)sum;
}

namespace {
struct Put {
  uint8_t *p;
  void u16(uint32_t v) {
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8);
    p += 2;
  }
  void u32(uint32_t v) {
    u16(v & 0xffff);
    u16(v >> 16);
  }
  void u64(uint64_t v) {
    u32((uint32_t)v);
    u32((uint32_t)(v >> 32));
  }
};
}  // namespace

static int zip_compress(md_ctx *ctx, int level, size_t n, const md_zip_source *files, const uint8_t *src, uint8_t *dst, size_t dst_cap, size_t *written) {
  std::vector<uint64_t> h_in_off(n), h_in_len(n), h_slot_off(n), h_name_pos(n), first;
  std::vector<uint32_t> h_name_len(n), h_dos(n), seg_entry;
  std::vector<uint8_t> names;
  uint64_t lo = UINT64_MAX, hi = 0, slots_bytes = 0, total_in = 0, dir_size = 0, longest = 0;
  for (size_t i = 0; i < n; i++) {
    if (files[i].len && files[i].off < lo) lo = files[i].off;
    if (files[i].len && files[i].off + files[i].len > hi) hi = files[i].off + files[i].len;
  }
  if (hi == 0) lo = 0;
  for (size_t i = 0; i < n; i++) {
    const md_zip_source &f = files[i];
    h_in_off[i] = f.len ? f.off - lo : 0;
    h_in_len[i] = f.len;
    h_slot_off[i] = slots_bytes;
    slots_bytes += (f.len + 15) & ~(uint64_t)15;
    h_name_pos[i] = names.size();
    h_name_len[i] = (uint32_t)f.name_len;
    h_dos[i] = (uint32_t)f.dos_time | (uint32_t)f.dos_date << 16;
    names.insert(names.end(), (const uint8_t *)f.name, (const uint8_t *)f.name + f.name_len);
    total_in += f.len;
    dir_size += 46 + f.name_len;
    if (f.len > longest) longest = f.len;
  }
  const uint64_t seg = ctx->zip_segment, image_max = total_in + 30 * (uint64_t)n + names.size();
  segment_table(h_in_len, seg, &first, &seg_entry);
  const size_t nseg = seg_entry.size(), span = (size_t)(hi - lo);

  MD_ON_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  uint64_t *in_off = nullptr, *in_len = nullptr, *slot_off = nullptr, *out_len = nullptr, *name_pos = nullptr, *lsize = nullptr, *loff = nullptr,
           *d_first = nullptr;
  int32_t *status = nullptr, *err = nullptr;
  uint32_t *name_len = nullptr, *dos = nullptr, *rec = nullptr, *d_seg_entry = nullptr, *crc = nullptr;
  uint8_t *kind = nullptr, *d_names = nullptr;
  int rc = carve(ctx, ctx->scratch[kZipDesc], "hipMalloc(zip descriptors)", [&](md::Carver &c) {
    in_off = c.take<uint64_t>(n);
    in_len = c.take<uint64_t>(n);
    slot_off = c.take<uint64_t>(n);
    out_len = c.take<uint64_t>(n);
    name_pos = c.take<uint64_t>(n);
    lsize = c.take<uint64_t>(n);
    loff = c.take<uint64_t>(n + 1);
    d_first = c.take<uint64_t>(n + 1);
    status = c.take<int32_t>(n);
    err = c.take<int32_t>(1);
    name_len = c.take<uint32_t>(n);
    dos = c.take<uint32_t>(n);
    rec = c.take<uint32_t>(4 * n);
    d_seg_entry = c.take<uint32_t>(nseg);
    crc = c.take<uint32_t>(nseg);
    kind = c.take<uint8_t>(n);
    d_names = c.take<uint8_t>(names.size());
  });
  if (rc == MD_OK) rc = upload_host_in(ctx, src + lo, span);
  if (rc == MD_OK) rc = ctx->scratch[kHostOut].reserve(ctx, (size_t)slots_bytes + 64, "hipMalloc(host path output)");
  if (rc == MD_OK) rc = ctx->scratch[kZipOut].reserve(ctx, (size_t)image_max + 64, "hipMalloc(zip file image)");
  if (rc != MD_OK) return rc;
  const uint8_t *d_in = (const uint8_t *)ctx->scratch[kHostIn].p;
  uint8_t *slots = (uint8_t *)ctx->scratch[kHostOut].p, *d_file = (uint8_t *)ctx->scratch[kZipOut].p;
  HIP_TRY(ctx, md::to_device(in_off, h_in_off, st));
  HIP_TRY(ctx, md::to_device(in_len, h_in_len, st));
  HIP_TRY(ctx, md::to_device(slot_off, h_slot_off, st));
  HIP_TRY(ctx, md::to_device(name_pos, h_name_pos, st));
  HIP_TRY(ctx, md::to_device(name_len, h_name_len, st));
  HIP_TRY(ctx, md::to_device(dos, h_dos, st));
  HIP_TRY(ctx, md::to_device(d_first, first, st));
  HIP_TRY(ctx, md::to_device(d_seg_entry, seg_entry, st));
  HIP_TRY(ctx, md::to_device(d_names, names, st));
  HIP_TRY(ctx, md::zero(err, 1, st));
  if (n) HIP_TRY(ctx, hipMemsetAsync(kind, md::zip::kStored, n, st));
  if (n && level != 0) {
    // the room of a file is its own length (in_len serves as out_cap): a body that is not shorter loses against stored
    const md_deflate_params p = gzip_body_params(level, (size_t)total_in);
    rc = md_deflate_batch_device(ctx, MD_FORMAT_DEFLATE, &p, n, d_in, in_off, in_len, slots, slot_off, in_len, out_len, status, nullptr);
    if (rc != MD_OK) return rc;
  }
  MD_LAUNCH_TRY(ctx, md_launch_zip_segments(nseg, seg, d_seg_entry, d_first, in_len, kind, d_in, in_off, nullptr, nullptr, crc, st));
  MD_LAUNCH_TRY(ctx, md_launch_zip_sizes(n, level, in_len, name_len, out_len, status, d_first, seg, crc, lsize, rec, err, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan64(lsize, n, loff, st));
  MD_LAUNCH_TRY(ctx, md_launch_zip_pack(n, longest, d_in, in_off, in_len, slots, slot_off, d_names, name_pos, name_len, dos, loff, rec, d_file, st));
  std::vector<uint32_t> h_rec(4 * n);
  uint64_t image = 0;
  int32_t bad = 0;
  HIP_TRY(ctx, md::to_host(h_rec.data(), rec, h_rec.size(), st));
  HIP_TRY(ctx, md::to_host(&image, loff + n, 1, st));
  HIP_TRY(ctx, md::to_host(&bad, err, 1, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (bad != 0) return bad;  // (MD_QUEUE_FULL: not with this queue, said all the same)
  if (image > image_max) return fail(ctx, MD_E_HIP, "zip: local sizes above the bound");
  const bool z64 = n >= kZip64From;
  const uint64_t total = image + dir_size + (z64 ? 76 : 0) + 22;
  if (total > dst_cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  if (image) HIP_TRY(ctx, hipMemcpy(dst, d_file, (size_t)image, hipMemcpyDeviceToHost));
  Put o{dst + image};
  for (size_t i = 0; i < n; i++) {
    const md_zip_source &f = files[i];
    const uint32_t method = h_rec[4 * i + 2];
    uint32_t utf8 = 0;
    for (size_t t = 0; t < f.name_len; t++) utf8 |= (uint8_t)f.name[t] & 0x80u;
    o.u32(md::zip::kSigCentral);
    o.u16(3 << 8 | 20);  // made by: Unix (external_attr holds its mode bits), 2.0
    o.u16(method ? 20 : 10);
    o.u16(utf8 ? 0x0800 : 0);
    o.u16(method);
    o.u16(f.dos_time);
    o.u16(f.dos_date);
    o.u32(h_rec[4 * i]);
    o.u32(h_rec[4 * i + 1]);
    o.u32((uint32_t)f.len);
    o.u16((uint32_t)f.name_len);
    o.u16(0);  // extra field, comment, disk, internal attributes
    o.u16(0);
    o.u16(0);
    o.u16(0);
    o.u32(f.external_attr);
    o.u32(h_rec[4 * i + 3]);
    memcpy(o.p, f.name, f.name_len);
    o.p += f.name_len;
  }
  if (z64) {
    o.u32(md::zip::kSigEnd64);
    o.u64(md::zip::kEndRecord64 - 12);
    o.u16(45);
    o.u16(45);
    o.u32(0);
    o.u32(0);
    o.u64(n);
    o.u64(n);
    o.u64(dir_size);
    o.u64(image);
    o.u32(md::zip::kSigLocator64);
    o.u32(0);
    o.u64(image + dir_size);
    o.u32(1);
  }
  o.u32(md::zip::kSigEnd);
  o.u16(0);
  o.u16(0);
  o.u16(z64 ? 0xffff : (uint32_t)n);
  o.u16(z64 ? 0xffff : (uint32_t)n);
  o.u32((uint32_t)dir_size);
  o.u32((uint32_t)image);
  o.u16(0);
  *written = (size_t)total;
  return MD_OK;
}

int md_zip_compress(md_ctx *ctx, int level, size_t n, const md_zip_source *files, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                    size_t *written) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!written || (!files && n) || (!src && src_len) || (!dst && dst_cap)) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  *written = 0;
  if (level < 0 || level > 9) return fail(ctx, MD_E_INVALID_ARGUMENT, "Invalid level of compression");
  if (n > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many files in one call");
  for (size_t i = 0; i < n; i++) {
    const md_zip_source &f = files[i];
    if (!f.name || f.name_len == 0 || f.name_len > 0xffff) return fail(ctx, MD_E_INVALID_ARGUMENT, "a file's name has 1 .. 65535 bytes");
    if (f.len > MD_MAX_STREAM || f.off > src_len || f.len > src_len - f.off) return fail(ctx, MD_E_INVALID_ARGUMENT, "a file beyond the source, or too long");
  }
  const size_t bound = md_zip_compress_bound(n, files);
  if (bound == 0 || bound >= ((uint64_t)1 << 32)) return fail(ctx, MD_E_INVALID_ARGUMENT, "the archive could reach 4 GiB: the writer has no 64-bit offsets");
  return no_bad_alloc(ctx, "host memory for the archive's descriptors", [&] { return zip_compress(ctx, level, n, files, src, dst, dst_cap, written); });
}
