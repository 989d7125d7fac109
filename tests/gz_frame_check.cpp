// gz_frame_check.cpp — csrc/gz_frame.hpp on its own, for a sanitizer build (test_gz_frame_check.py compiles this with
// -fsanitize=address,undefined and runs it alone).  It reads a file of cases, in zindex_check.cpp's form:
//   B <hex bytes>          a base frame (numbered from 0 in order of appearance)
//   T <base> <length>      the base cut to `length` bytes
//   M <base> <pos> <value> the base with byte `pos` set to `value`
// and prints one line per case: status, body offset, offset and length of extra, name and comment, flg, mtime, xfl, os.
// Every case is walked in a heap block of exactly its length, so a read past the end is a finding.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "gz_frame.hpp"

static void run(const uint8_t *bytes, size_t len) {
  uint8_t *p = (uint8_t *)malloc(len ? len : 1);
  if (len) memcpy(p, bytes, len);
  md::gz::InfHeader h;
  const int st = md::gz::inf_header(p, len, &h);
  printf("%d %zu %zu %zu %zu %zu %zu %zu %u %u %u %u\n", st, h.body, h.extra_off, h.extra_len, h.name_off, h.name_len, h.comment_off,
         h.comment_len, h.flg, h.mtime, h.xfl, h.os);
  free(p);
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
      run(b.data(), b.size());
    }
    line.clear();
  }
  fclose(f);
  return 0;
}
