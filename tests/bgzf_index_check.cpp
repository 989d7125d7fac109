// bgzf_index_check.cpp — csrc/bgzf_index.hpp on its own, for a sanitizer build (test_bgzf_index_check.py compiles this with
// -fsanitize=address,undefined and runs it alone).  It reads a file of cases, in gz_frame_check.cpp's form:
//   S <hex bytes>          the file the blobs index (once, first)
//   B <hex bytes>          a base .gzi blob (numbered from 0 in order of appearance)
//   T <base> <length>      the base cut to `length` bytes
//   M <base> <pos> <value> the base with byte `pos` set to `value`
//   C <length>             base 0 whole, against the file cut to `length` bytes
// and prints one line per case: status, members, size, and the bytes to_gzi makes of the index (hex; "-" without one).
// Blob and file each lie in a heap block of exactly their length, so a read past the end is a finding.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "bgzf_index.hpp"

static uint8_t *exact(const std::vector<uint8_t> &b, size_t len) {
  uint8_t *p = (uint8_t *)malloc(len ? len : 1);
  if (len) memcpy(p, b.data(), len);
  return p;
}

static void run(const std::vector<uint8_t> &blob, const std::vector<uint8_t> &file, size_t file_len) {
  uint8_t *g = exact(blob, blob.size()), *s = exact(file, file_len);
  md_bgzf_index *x = nullptr;
  const int st = md::bgzf::from_gzi(g, blob.size(), s, file_len, &x);
  if ((st == MD_OK) != (x != nullptr)) abort();
  if (!x) printf("%d 0 0 -\n", st);
  else {
    printf("%d %zu %llu ", st, x->members(), (unsigned long long)x->size());
    std::vector<uint8_t> out(md::bgzf::gzi_size(x));
    md::bgzf::to_gzi(x, out.data());
    for (uint8_t b : out) printf("%02x", b);
    printf("\n");
    delete x;
  }
  free(g);
  free(s);
}

static std::vector<uint8_t> unhex(const std::string &line) {
  std::vector<uint8_t> b;
  for (size_t i = 2; i + 1 < line.size(); i += 2) b.push_back((uint8_t)strtoul(line.substr(i, 2).c_str(), nullptr, 16));
  return b;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<uint8_t> file;
  std::vector<std::vector<uint8_t>> bases;
  std::string line;
  int c;
  while ((c = fgetc(f)) != EOF) {
    if (c != '\n') {
      line.push_back((char)c);
      continue;
    }
    if (line.size() >= 2 && line[0] == 'S') file = unhex(line);
    else if (line.size() >= 2 && line[0] == 'B') bases.push_back(unhex(line));
    else if (!line.empty()) {
      unsigned long base = 0, a = 0, v = 0;
      char kind = 0;
      const int got = sscanf(line.c_str(), "%c %lu %lu %lu", &kind, &base, &a, &v);
      if (kind == 'C' && got == 2 && !bases.empty() && base <= file.size()) run(bases[0], file, base);
      else {
        if (got < 3 || base >= bases.size()) return 3;
        std::vector<uint8_t> b = bases[base];
        if (kind == 'T' && a <= b.size()) b.resize(a);
        else if (kind == 'M' && got == 4 && a < b.size()) b[a] = (uint8_t)v;
        else return 3;
        run(b, file, file.size());
      }
    }
    line.clear();
  }
  fclose(f);
  return 0;
}
