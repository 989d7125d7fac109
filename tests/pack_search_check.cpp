// pack_search_check.cpp — csrc/pack_search.hpp on its own, for a sanitizer build (test_pack_search_check.py compiles this with
// -fsanitize=address,undefined and runs it alone).  It reads a file of cases and prints one line per case:
//   G <len>                                                      -> "<positions> <segments>"
//   C <window> <n> then n x (<type> <len> <f0> <f1> <f2> <f3>)   -> the order, then " |", then the pairs as "<target>:<base>"
//   S <window> <max_depth> <n> then the n objects as above, then <pairs> then pairs x (<fitted> <len>)
//                                                                -> "<chosen>" then n x "<base>:<depth>"
// Ranks throughout; base -1: none.  Every array lives in a heap block of exactly its length, so a step past an end is a finding.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pack_search.hpp"

template <class T>
static T *exact(size_t n) {
  return (T *)calloc(n ? n : 1, n ? sizeof(T) : 1);
}

struct Objects {
  size_t n;
  md_pack_source *objs;
  uint32_t *features;
  uint64_t *order;
};

static Objects read_objects(char *&p) {
  Objects o;
  o.n = strtoull(p, &p, 10);
  o.objs = exact<md_pack_source>(o.n), o.features = exact<uint32_t>(o.n * md::pks::kFeatures), o.order = exact<uint64_t>(o.n);
  for (size_t i = 0; i < o.n; i++) {
    o.objs[i].type = (uint32_t)strtoul(p, &p, 10), o.objs[i].len = strtoull(p, &p, 10);
    o.objs[i].off = 0, o.objs[i].base = 12345;  // (base is not looked at)
    for (uint32_t k = 0; k < md::pks::kFeatures; k++) o.features[md::pks::kFeatures * i + k] = (uint32_t)strtoul(p, &p, 10);
  }
  md::pks::pack_order(o.n, o.objs, o.order);
  return o;
}

static void free_objects(Objects &o) { free(o.objs), free(o.features), free(o.order); }

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
    if (kind == 'G') {
      const uint64_t len = strtoull(p, &p, 10);
      printf("%llu %llu\n", (unsigned long long)md::pks::positions(len), (unsigned long long)md::pks::segments(len));
    } else if (kind == 'C' || kind == 'S') {
      const uint32_t window = (uint32_t)strtoul(p, &p, 10);
      const uint32_t max_depth = kind == 'S' ? (uint32_t)strtoul(p, &p, 10) : 0;
      Objects o = read_objects(p);
      md::pks::Pairs pairs;
      md::pks::candidates(o.n, o.objs, o.order, o.features, window, &pairs);
      if (pairs.first.size() != o.n + 1 || pairs.first[o.n] != pairs.base.size()) return 4;
      if (kind == 'C') {
        for (size_t r = 0; r < o.n; r++) printf("%s%llu", r ? " " : "", (unsigned long long)o.order[r]);
        printf(" |");
        for (size_t t = 0; t < o.n; t++)
          for (uint64_t k = pairs.first[t]; k < pairs.first[t + 1]; k++) printf(" %zu:%u", t, pairs.base[k]);
        printf("\n");
      } else {
        const size_t np = strtoull(p, &p, 10);
        if (np != pairs.base.size()) return 5;
        uint64_t *len = exact<uint64_t>(np), *base = exact<uint64_t>(o.n);
        uint8_t *fitted = exact<uint8_t>(np);
        uint32_t *depth = exact<uint32_t>(o.n);
        for (size_t k = 0; k < np; k++) fitted[k] = (uint8_t)strtoul(p, &p, 10), len[k] = strtoull(p, &p, 10);
        const uint64_t chosen = md::pks::choose(o.n, pairs, len, fitted, max_depth, base, depth);
        printf("%llu", (unsigned long long)chosen);
        for (size_t r = 0; r < o.n; r++) printf(" %lld:%u", base[r] == MD_PACK_NO_BASE ? -1ll : (long long)base[r], depth[r]);
        printf("\n");
        free(len), free(base), free(fitted), free(depth);
      }
      free_objects(o);
    } else if (kind) {
      return 3;
    }
    line.clear();
  }
  fclose(f);
  return 0;
}
