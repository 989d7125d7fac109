// carver_check.cpp — md::Carver (csrc/host_util.hpp) on its own, for a sanitizer build (test_carver_check.py compiles
// this with -fsanitize=address,undefined and runs it alone).  It reads a file of lists, one a line, each a series of
// pairs "element-size count" with element sizes 1, 2, 4, 8 and 48.  For every list: the sizing pass over a null base, a
// heap block of exactly `at` bytes, the pointer pass over it, and a write to every element of every array - so an array
// that reaches past the block is a finding.  It prints the block's size per list, or says what is wrong and ends with 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "host_util.hpp"

namespace {
struct E48 {
  uint8_t b[48];
};
struct Want {
  size_t esize, count;
};

uint8_t *take(md::Carver &c, const Want &w) {
  switch (w.esize) {
    case 1: return (uint8_t *)c.take<uint8_t>(w.count);
    case 2: return (uint8_t *)c.take<uint16_t>(w.count);
    case 4: return (uint8_t *)c.take<uint32_t>(w.count);
    case 8: return (uint8_t *)c.take<uint64_t>(w.count);
    case 48: return (uint8_t *)c.take<E48>(w.count);
  }
  return nullptr;
}

int fail(size_t line, const char *what) {
  fprintf(stderr, "list %zu: %s\n", line, what);
  return 1;
}

int run(size_t line, const std::vector<Want> &list) {
  md::Carver size;
  for (const Want &w : list)
    if (take(size, w) != nullptr) return fail(line, "the sizing pass handed out a pointer");
  uint8_t *block = (uint8_t *)malloc(size.at);
  md::Carver c(block);
  std::vector<uint8_t *> at;
  for (const Want &w : list) at.push_back(take(c, w));
  if (c.at != size.at) return fail(line, "the two passes end at different sizes");
  for (size_t i = 0; i < list.size(); i++) {
    const size_t bytes = list[i].esize * list[i].count;
    if (!at[i]) {
      if (block) return fail(line, "a null array over a block");
      continue;
    }
    if ((uintptr_t)at[i] % 16 != 0 || (size_t)(at[i] - block) % 16 != 0) return fail(line, "an array off 16 bytes");
    if (at[i] < block || (size_t)(at[i] - block) + bytes > size.at) return fail(line, "an array outside the block");
    // (the arrays come in order: each begins at or behind the end of the one before)
    if (i && at[i - 1] && at[i] < at[i - 1] + list[i - 1].esize * list[i - 1].count) return fail(line, "two arrays overlap");
    for (size_t k = 0; k < list[i].count; k++) memset(at[i] + k * list[i].esize, (int)(i + 1), list[i].esize);
  }
  for (size_t i = 0; i < list.size(); i++)  // every element still holds its own array's mark
    for (size_t b = 0; at[i] && b < list[i].esize * list[i].count; b++)
      if (at[i][b] != (uint8_t)(i + 1)) return fail(line, "an array was written over");
  free(block);
  printf("%zu\n", size.at);
  return 0;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  char buf[1 << 16];
  size_t line = 0;
  while (fgets(buf, sizeof buf, f)) {
    std::istringstream in(buf);
    std::vector<Want> list;
    Want w;
    while (in >> w.esize >> w.count) {
      if (w.esize != 1 && w.esize != 2 && w.esize != 4 && w.esize != 8 && w.esize != 48) return 3;
      list.push_back(w);
    }
    if (run(line++, list) != 0) return 1;
  }
  fclose(f);
  return 0;
}
