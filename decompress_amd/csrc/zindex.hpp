// zindex.hpp — the index of one long DEFLATE / ZLIB / GZip stream (mdeflate.h: md_inflate_index_*): access points at
// block starts, each with its bit offset, its output offset and the window in front of it; and its serialised form.
// Plain C++: no HIP, no md_ctx.  `load` checks everything a later read trusts, and reads no byte of the blob before it
// has checked that the byte is there.  The layout is in mdeflate.h, byte by byte.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "mdeflate.h"

struct md_inflate_index {
  md_inflate_index_info info = {};
  std::vector<uint64_t> bit, out;  // [points]
  std::vector<uint64_t> win_off;   // [points + 1]: window k is wins[win_off[k], win_off[k + 1])
  std::vector<uint8_t> wins;       // the windows back to back
};

namespace md {
namespace zix {

constexpr uint64_t kWindow = 32768, kHeadBytes = 72, kPointBytes = 24, kSpanMin = 4096, kSpanDefault = (uint64_t)1 << 20;
constexpr uint32_t kVersion = 1;
constexpr uint8_t kMagic[8] = {'M', 'D', 'Z', 'I', 'N', 'D', 'E', 'X'};

inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t rd64(const uint8_t *p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }
inline void wr32(uint8_t *p, uint32_t v) {
  for (int k = 0; k < 4; k++) p[k] = (uint8_t)(v >> (8 * k));
}
inline void wr64(uint8_t *p, uint64_t v) {
  wr32(p, (uint32_t)v);
  wr32(p + 4, (uint32_t)(v >> 32));
}

inline uint64_t trailer_len(int format) { return format == MD_FORMAT_ZLIB ? 4 : format == MD_FORMAT_GZIP ? 8 : 0; }
inline uint64_t window_len(uint64_t out) { return out < kWindow ? out : kWindow; }

// one more point: its window is the w = window_len(out) bytes at win
inline void add_point(md_inflate_index *x, uint64_t bit, uint64_t out, const uint8_t *win) {
  if (x->win_off.empty()) x->win_off.push_back(0);
  x->bit.push_back(bit);
  x->out.push_back(out);
  const uint64_t w = window_len(out);
  if (w) x->wins.insert(x->wins.end(), win, win + w);
  x->win_off.push_back(x->wins.size());
  x->info.points = x->bit.size();
}

inline size_t save_size(const md_inflate_index *x) { return (size_t)(kHeadBytes + kPointBytes * x->bit.size() + x->wins.size()); }

inline void save(const md_inflate_index *x, uint8_t *buf) {
  const md_inflate_index_info &f = x->info;
  memcpy(buf, kMagic, 8);
  wr32(buf + 8, kVersion);
  wr32(buf + 12, (uint32_t)f.format);
  wr64(buf + 16, f.src_len);
  wr64(buf + 24, f.header_len);
  wr64(buf + 32, f.consumed);
  wr64(buf + 40, f.size);
  wr64(buf + 48, f.span);
  wr64(buf + 56, f.points);
  wr32(buf + 64, f.checksum);
  wr32(buf + 68, 0);
  uint8_t *p = buf + kHeadBytes;
  for (size_t k = 0; k < x->bit.size(); k++, p += kPointBytes) {
    wr64(p, x->bit[k]);
    wr64(p + 8, x->out[k]);
    wr32(p + 16, (uint32_t)(x->win_off[k + 1] - x->win_off[k]));
    wr32(p + 20, 0);
  }
  if (!x->wins.empty()) memcpy(p, x->wins.data(), x->wins.size());
}

// MD_OK and *res (the caller's to delete), MD_INVALID_INDEX, or MD_E_OUT_OF_MEMORY
inline int load(const uint8_t *buf, size_t len, md_inflate_index **res) {
  *res = nullptr;
  if (len < kHeadBytes || memcmp(buf, kMagic, 8) != 0 || rd32(buf + 8) != kVersion || rd32(buf + 68) != 0) return MD_INVALID_INDEX;
  md_inflate_index_info f;
  const uint32_t format = rd32(buf + 12);
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP) return MD_INVALID_INDEX;
  f.format = (int32_t)format;
  f.src_len = rd64(buf + 16);
  f.header_len = rd64(buf + 24);
  f.consumed = rd64(buf + 32);
  f.size = rd64(buf + 40);
  f.span = rd64(buf + 48);
  f.points = rd64(buf + 56);
  f.checksum = rd32(buf + 64);
  const uint64_t trailer = trailer_len(f.format);
  // the frame: header, body, trailer inside src (bit offsets are 64-bit: eight times a length must fit)
  if (f.src_len >> 60 || f.consumed > f.src_len || f.header_len > f.consumed || f.consumed - f.header_len < trailer) return MD_INVALID_INDEX;
  if (f.format == MD_FORMAT_DEFLATE ? f.header_len != 0 : f.format == MD_FORMAT_ZLIB ? f.header_len != 2 : f.header_len < 10)
    return MD_INVALID_INDEX;
  if (f.span < kSpanMin) return MD_INVALID_INDEX;
  const uint64_t room = len - kHeadBytes;
  if (f.points < 1 || f.points > room / kPointBytes) return MD_INVALID_INDEX;  // (also bounds what is allocated)
  const size_t P = (size_t)f.points;
  md_inflate_index *x = new (std::nothrow) md_inflate_index();
  if (!x) return MD_E_OUT_OF_MEMORY;
  int rc = MD_OK;
  try {
    x->bit.resize(P);
    x->out.resize(P);
    x->win_off.resize(P + 1);
  } catch (const std::bad_alloc &) {
    rc = MD_E_OUT_OF_MEMORY;
  }
  uint64_t wins = 0;
  const uint8_t *p = buf + kHeadBytes;
  for (size_t k = 0; rc == MD_OK && k < P; k++, p += kPointBytes) {
    const uint64_t bit = rd64(p), out = rd64(p + 8), w = rd32(p + 16);
    bool ok = rd32(p + 20) == 0 && w == window_len(out) && bit >= 8 * f.header_len && bit < 8 * (f.consumed - trailer);
    ok = ok && (k == 0 ? bit == 8 * f.header_len && out == 0 : bit > x->bit[k - 1] && out > x->out[k - 1]);
    ok = ok && (out < f.size || (out == f.size && k + 1 == P));  // (the last point may be an empty block at the very end)
    if (!ok) rc = MD_INVALID_INDEX;
    x->bit[k] = bit;
    x->out[k] = out;
    x->win_off[k] = wins;
    wins += w;
  }
  if (rc == MD_OK && wins != room - kPointBytes * f.points) rc = MD_INVALID_INDEX;  // exactly as long as it says: no trailing bytes
  if (rc == MD_OK) {
    x->win_off[P] = wins;
    try {
      x->wins.assign(p, p + wins);
    } catch (const std::bad_alloc &) {
      rc = MD_E_OUT_OF_MEMORY;
    }
  }
  if (rc != MD_OK) {
    delete x;
    return rc;
  }
  x->info = f;
  *res = x;
  return MD_OK;
}

}  // namespace zix
}  // namespace md
