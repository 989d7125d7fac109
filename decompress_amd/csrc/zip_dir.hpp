// zip_dir.hpp — the directory of a ZIP archive (PKWARE APPNOTE 4.3-4.5), read on the host: end record, ZIP64 end record
// with its locator, central directory headers.  Plain C++: no HIP, no md_ctx.  Every read of src is checked against
// src_len first, and no offset taken from the file is used before it is checked.  The rules are in mdeflate.h
// (md_zip_directory); they are Python zipfile's reading, with one difference: the end record must fit the end of the file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "mdeflate.h"

namespace md {
namespace zip {

constexpr uint64_t kEndRecord = 22, kEndRecord64 = 56, kLocator64 = 20, kCentralHeader = 46, kLocalHeader = 30;
constexpr uint32_t kSigEnd = 0x06054b50u, kSigEnd64 = 0x06064b50u, kSigLocator64 = 0x07064b50u, kSigCentral = 0x02014b50u,
                   kSigLocal = 0x04034b50u;

inline uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }
inline uint64_t rd64(const uint8_t *p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }

// the ZIP64 extra field 0x0001 of the extra fields x[0, xlen): its payload, or null
inline const uint8_t *zip64_extra(const uint8_t *x, uint64_t xlen, uint64_t *payload_len) {
  uint64_t q = 0;
  while (xlen - q >= 4) {
    const uint64_t id = rd16(x + q), sz = rd16(x + q + 2);
    if (sz > xlen - q - 4) return nullptr;
    if (id == 1) {
      *payload_len = sz;
      return x + q + 4;
    }
    q += 4 + sz;
  }
  return nullptr;
}

inline int read_directory(const uint8_t *src, size_t src_len, md_zip_info *info, md_zip_entry *entries, size_t cap) {
  const uint64_t len = src_len;
  memset(info, 0, sizeof *info);
  if (len < kEndRecord) return MD_INVALID_ZIP_DIRECTORY;
  // the last end record whose comment ends with the file
  const uint64_t lowest = len > kEndRecord + 0xffff ? len - kEndRecord - 0xffff : 0;
  uint64_t p = len - kEndRecord;
  for (;; p--) {
    if (rd32(src + p) == kSigEnd && p + kEndRecord + rd16(src + p + 20) == len) break;
    if (p == lowest) return MD_INVALID_ZIP_DIRECTORY;
  }
  uint64_t disk = rd16(src + p + 4), dir_disk = rd16(src + p + 6), here = rd16(src + p + 8), count = rd16(src + p + 10),
           dir_size = rd32(src + p + 12), dir_off = rd32(src + p + 16), end = p;
  const bool z64 = p >= kLocator64 && rd32(src + p - kLocator64) == kSigLocator64;
  if (z64) {
    const uint8_t *loc = src + p - kLocator64;
    if (p < kLocator64 + kEndRecord64) return MD_INVALID_ZIP_DIRECTORY;
    const uint8_t *r = loc - kEndRecord64;
    if (rd32(r) != kSigEnd64 || rd64(r + 4) != kEndRecord64 - 12) return MD_INVALID_ZIP_DIRECTORY;
    if ((disk != 0 && disk != 0xffff) || (dir_disk != 0 && dir_disk != 0xffff)) return MD_INVALID_ZIP_DIRECTORY;
    if (rd32(loc + 4) != 0 || rd32(loc + 16) > 1) return MD_INVALID_ZIP_DIRECTORY;  // (disk of the record; disks in all)
    disk = rd32(r + 16);
    dir_disk = rd32(r + 20);
    here = rd64(r + 24);
    count = rd64(r + 32);
    dir_size = rd64(r + 40);
    dir_off = rd64(r + 48);
    end = p - kLocator64 - kEndRecord64;
  }
  if (disk != 0 || dir_disk != 0 || here != count) return MD_INVALID_ZIP_DIRECTORY;
  if (dir_size > end || dir_off > end - dir_size) return MD_INVALID_ZIP_DIRECTORY;
  if (count > dir_size / kCentralHeader) return MD_INVALID_ZIP_DIRECTORY;  // (also bounds what a caller allocates)
  const uint64_t prefix = end - dir_size - dir_off, dir_end = end;
  uint64_t q = end - dir_size, total = 0;
  for (uint64_t i = 0; i < count; i++) {
    if (dir_end - q < kCentralHeader) return MD_INVALID_ZIP_DIRECTORY;
    const uint8_t *h = src + q;
    if (rd32(h) != kSigCentral) return MD_INVALID_ZIP_DIRECTORY;
    const uint64_t n = rd16(h + 28), e = rd16(h + 30), c = rd16(h + 32);
    if (dir_end - q - kCentralHeader < n + e + c) return MD_INVALID_ZIP_DIRECTORY;
    uint64_t csize = rd32(h + 20), usize = rd32(h + 24), edisk = rd16(h + 34), off = rd32(h + 42);
    if (usize == 0xffffffffu || csize == 0xffffffffu || off == 0xffffffffu || edisk == 0xffff) {
      uint64_t have = 0, at = 0;
      const uint8_t *x = zip64_extra(h + kCentralHeader + n, e, &have);
      if (!x) return MD_INVALID_ZIP_DIRECTORY;
      uint64_t *const field[3] = {&usize, &csize, &off};
      for (int k = 0; k < 3; k++) {
        if (*field[k] != 0xffffffffu) continue;
        if (have - at < 8) return MD_INVALID_ZIP_DIRECTORY;
        *field[k] = rd64(x + at);
        at += 8;
      }
      if (edisk == 0xffff) {
        if (have - at < 4) return MD_INVALID_ZIP_DIRECTORY;
        edisk = rd32(x + at);
      }
    }
    if (edisk != 0 || off + prefix < off || total + usize < total) return MD_INVALID_ZIP_DIRECTORY;
    total += usize;
    if (i < cap) {
      md_zip_entry *o = entries + i;
      memset(o, 0, sizeof *o);
      o->header_off = off + prefix;
      o->csize = csize;
      o->usize = usize;
      o->name_off = q + kCentralHeader;
      o->crc32 = rd32(h + 16);
      o->external_attr = rd32(h + 38);
      o->name_len = (uint16_t)n;
      o->method = (uint16_t)rd16(h + 10);
      o->flags = (uint16_t)rd16(h + 8);
      o->dos_time = (uint16_t)rd16(h + 12);
      o->dos_date = (uint16_t)rd16(h + 14);
    }
    q += kCentralHeader + n + e + c;
  }
  if (q != dir_end) return MD_INVALID_ZIP_DIRECTORY;
  info->entries = (size_t)count;
  info->total_usize = total;
  info->dir_off = dir_off;
  info->dir_size = dir_size;
  info->prefix = prefix;
  info->comment_off = p + kEndRecord;
  info->comment_len = (uint32_t)(len - p - kEndRecord);
  info->zip64 = z64 ? 1 : 0;
  return MD_OK;
}

}  // namespace zip
}  // namespace md
