// pack_index_check.cpp — csrc/pack_index.hpp on its own, for a sanitizer build (test_pack_index_check.py compiles this with
// -fsanitize=address,undefined and runs it alone).  It reads a file of cases and prints one status per case:
//   B <hex bytes>          a base idx (numbered from 0 in order of appearance)
//   T <base> <length>      the base cut to `length` bytes
//   M <base> <pos> <value> the base with byte `pos` set to `value`
// Every case is parsed from a heap block of exactly its length, so a read past the end is a finding; the entries go into
// a block of exactly `n` records, and every name the idx holds is looked up again through find_name.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pack_index.hpp"

static int run(const uint8_t *bytes, size_t len) {
  uint8_t *p = (uint8_t *)malloc(len ? len : 1);
  if (len) memcpy(p, bytes, len);
  md_pack_index_info info;
  int st = md::pack::read_index(p, len, &info, nullptr, 0);
  if (st == MD_OK) {
    md_pack_index_entry *e = (md_pack_index_entry *)malloc((size_t)info.n * sizeof(md_pack_index_entry) + 1);
    const int again = md::pack::read_index(p, len, &info, e, (size_t)info.n);
    if (again != st) st = 1000 + again;  // (never: the two passes read the same bytes)
    uint32_t fan[256];
    for (int b = 0; b < 256; b++) fan[b] = md::pack::be32(p + 8 + 4 * b);
    for (uint64_t i = 0; i < info.n && st == MD_OK; i++)
      if (md::pack::find_name(e[0].name, sizeof(md_pack_index_entry), fan, e[i].name) != (int64_t)i) st = 2000;
    free(e);
  }
  free(p);
  return st;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<std::vector<uint8_t>> bases;
  std::string line;
  int c;
  while ((c = fgetc(f)) != EOF) {
    if (c != '\n') {
      line.push_back((char)c);
      continue;
    }
    if (line.size() >= 2 && line[0] == 'B') {
      std::vector<uint8_t> b;
      for (size_t i = 2; i + 1 < line.size(); i += 2) b.push_back((uint8_t)strtoul(line.substr(i, 2).c_str(), nullptr, 16));
      bases.push_back(b);
    } else if (!line.empty()) {
      unsigned long base = 0, a = 0, v = 0;
      char kind = 0;
      const int got = sscanf(line.c_str(), "%c %lu %lu %lu", &kind, &base, &a, &v);
      if (got < 3 || base >= bases.size()) return 3;
      std::vector<uint8_t> b = bases[base];
      if (kind == 'T' && a <= b.size()) b.resize(a);
      else if (kind == 'M' && got == 4 && a < b.size()) b[a] = (uint8_t)v;
      else return 3;
      printf("%d\n", run(b.data(), b.size()));
    }
    line.clear();
  }
  fclose(f);
  return 0;
}
