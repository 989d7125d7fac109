// zindex_check.cpp — csrc/zindex.hpp on its own, for a sanitizer build (test_zindex_check.py compiles this with
// -fsanitize=address,undefined and runs it alone).  It reads a file of cases and prints one status per case:
//   B <hex bytes>          a base blob (numbered from 0 in order of appearance)
//   T <base> <length>      the base cut to `length` bytes
//   M <base> <pos> <value> the base with byte `pos` set to `value`
// Every case is loaded from a heap block of exactly its length, so a read past the end is a finding; a blob that loads is
// saved into a block of exactly its size and has to come back byte for byte.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "zindex.hpp"

static int run(const uint8_t *bytes, size_t len) {
  uint8_t *p = (uint8_t *)malloc(len ? len : 1);
  if (len) memcpy(p, bytes, len);
  md_inflate_index *x = nullptr;
  int st = md::zix::load(p, len, &x);
  if (st == MD_OK) {
    const size_t n = md::zix::save_size(x);
    uint8_t *q = (uint8_t *)malloc(n ? n : 1);
    md::zix::save(x, q);
    if (n != len || memcmp(p, q, len) != 0) st = 1000;  // (never: what loads is in canonical form)
    free(q);
    delete x;
  } else if (x) {
    st = 1001;
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
