// pack_write_check.cpp — csrc/pack_write.hpp on its own, for a sanitizer build (test_pack_write_check.py compiles this with
// -fsanitize=address,undefined and runs it alone).  It reads a file of cases and prints one line per case:
//   T <blocks>                                          -> table_bits
//   H <type> <size>                                     -> the object header's bytes in hex
//   O <distance>                                        -> the OFS_DELTA distance's bytes in hex
//   P <n> then n x <base len>                           -> "<blocks> <table words>" then n x "<table_off>:<first_block>:<bits>"
//   B <n> then n x <len>                                -> write_bound
//   K <max_depth> <n> then n x (<base> <tried> <fitted>) -> "<kept> <dropped_size> <dropped_depth>" then n x "<keep>:<depth>"
//   W <n> then n x (<type> <size> <base> <keep> <zlen>)  -> offset[n] then n x "<offset>:<header bytes in hex>"
// base: an index, or -1 for none.  Every array lives in a heap block of exactly its length, so a step past an end is a finding.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pack_write.hpp"

template <class T>
static T *exact(size_t n) {
  return (T *)calloc(n ? n : 1, n ? sizeof(T) : 1);
}

static void hex(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  std::string line;
  int ch;
  while ((ch = fgetc(f)) != EOF) {
    if (ch != '\n') {
      line.push_back((char)ch);
      continue;
    }
    char *p = line.size() > 1 ? &line[1] : nullptr;
    const char kind = line.empty() ? 0 : line[0];
    if (kind == 'T') {
      printf("%u\n", md::pkw::table_bits(strtoull(p, &p, 10)));
    } else if (kind == 'H') {
      const uint32_t type = (uint32_t)strtoul(p, &p, 10);
      const uint64_t size = strtoull(p, &p, 10);
      uint8_t *out = exact<uint8_t>(10);
      hex(out, md::pkw::object_header(type, size, out));
      printf("\n");
      free(out);
    } else if (kind == 'O') {
      uint8_t *out = exact<uint8_t>(10);
      hex(out, md::pkw::ofs_varint(strtoull(p, &p, 10), out));
      printf("\n");
      free(out);
    } else if (kind == 'P') {
      const size_t n = strtoull(p, &p, 10);
      md::pkw::TablePlace *at = exact<md::pkw::TablePlace>(n);
      md::pkw::TableRoom room;
      for (size_t i = 0; i < n; i++) at[i] = room.add(strtoull(p, &p, 10));
      printf("%llu %llu", (unsigned long long)room.blocks, (unsigned long long)room.words);
      for (size_t i = 0; i < n; i++) printf(" %llu:%llu:%u", (unsigned long long)at[i].table_off, (unsigned long long)at[i].first_block, at[i].bits);
      printf("\n");
      free(at);
    } else if (kind == 'B') {
      const size_t n = strtoull(p, &p, 10);
      md_pack_source *objs = exact<md_pack_source>(n);
      for (size_t i = 0; i < n; i++) objs[i].len = strtoull(p, &p, 10);
      printf("%llu\n", (unsigned long long)md::pkw::write_bound(n, objs));
      free(objs);
    } else if (kind == 'K') {
      const uint32_t max_depth = (uint32_t)strtoul(p, &p, 10);
      const size_t n = strtoull(p, &p, 10);
      uint64_t *base = exact<uint64_t>(n);
      uint8_t *tried = exact<uint8_t>(n), *fitted = exact<uint8_t>(n), *keep = exact<uint8_t>(n);
      uint32_t *depth = exact<uint32_t>(n);
      for (size_t i = 0; i < n; i++) {
        const long long b = strtoll(p, &p, 10);
        base[i] = b < 0 ? MD_PACK_NO_BASE : (uint64_t)b;
        tried[i] = (uint8_t)strtoul(p, &p, 10), fitted[i] = (uint8_t)strtoul(p, &p, 10);
      }
      const md::pkw::Kept k = md::pkw::keep_rule(n, base, tried, fitted, max_depth, keep, depth);
      printf("%llu %llu %llu", (unsigned long long)k.kept, (unsigned long long)k.dropped_size, (unsigned long long)k.dropped_depth);
      for (size_t i = 0; i < n; i++) printf(" %u:%u", keep[i], depth[i]);
      printf("\n");
      free(base), free(tried), free(fitted), free(keep), free(depth);
    } else if (kind == 'W') {
      const size_t n = strtoull(p, &p, 10);
      uint32_t *type = exact<uint32_t>(n);
      uint64_t *size = exact<uint64_t>(n), *base = exact<uint64_t>(n), *zlen = exact<uint64_t>(n), *offset = exact<uint64_t>(n + 1);
      uint8_t *keep = exact<uint8_t>(n), *head = exact<uint8_t>(n * md::pkw::kHeaderMax), *head_len = exact<uint8_t>(n);
      for (size_t i = 0; i < n; i++) {
        type[i] = (uint32_t)strtoul(p, &p, 10), size[i] = strtoull(p, &p, 10);
        const long long b = strtoll(p, &p, 10);
        base[i] = b < 0 ? MD_PACK_NO_BASE : (uint64_t)b;
        keep[i] = (uint8_t)strtoul(p, &p, 10), zlen[i] = strtoull(p, &p, 10);
      }
      md::pkw::walk_offsets(n, type, size, base, keep, zlen, offset, head, head_len);
      printf("%llu", (unsigned long long)offset[n]);
      for (size_t i = 0; i < n; i++) {
        printf(" %llu:", (unsigned long long)offset[i]);
        hex(head + md::pkw::kHeaderMax * i, head_len[i]);
      }
      printf("\n");
      free(type), free(size), free(base), free(zlen), free(offset), free(keep), free(head), free(head_len);
    } else if (kind) {
      return 3;
    }
    line.clear();
  }
  fclose(f);
  return 0;
}
