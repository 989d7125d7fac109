// host_steps_check.cpp — md::running_offsets and md::adjacent_runs (csrc/host_util.hpp) on their own, for a sanitizer build
// (test_host_steps_check.py compiles this with -fsanitize=address,undefined and runs it alone).  It reads a file of cases,
// one a line:
//   O k size_0 .. size_{k-1}                      prints  O total off_0 .. off_k
//   R n (status len dst_off) x n                  prints  R first bytes first bytes ..   (a pair per run)
// Every array lives on the heap at exactly its length, so a read or write past it is a finding.
#include <stdint.h>
#include <stdio.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "host_util.hpp"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    char kind = 0;
    size_t n = 0;
    if (!(in >> kind >> n)) return 3;
    if (kind == 'O') {
      std::vector<uint64_t> size(n), off(n + 1, 0x5555555555555555ull);
      for (uint64_t &s : size)
        if (!(in >> s)) return 3;
      const uint64_t total = md::running_offsets(n, off.data(), [&](size_t j) { return size[j]; });
      printf("O %llu", (unsigned long long)total);
      for (uint64_t o : off) printf(" %llu", (unsigned long long)o);
      printf("\n");
    } else if (kind == 'R') {
      std::vector<int32_t> status(n);
      std::vector<uint64_t> len(n), dst_off(n);
      for (size_t i = 0; i < n; i++)
        if (!(in >> status[i] >> len[i] >> dst_off[i])) return 3;
      printf("R");
      size_t calls = 0;
      const int rc = md::adjacent_runs(n, status.data(), len.data(), dst_off.data(), [&](size_t first, uint64_t bytes) {
        printf(" %zu %llu", first, (unsigned long long)bytes);
        calls++;
        return 0;
      });
      printf("\n");
      if (rc != 0) return 1;
      // a callback that refuses ends the walk there, and its word is the walk's
      size_t seen = 0;
      const int stop = md::adjacent_runs(n, status.data(), len.data(), dst_off.data(), [&](size_t, uint64_t) { return ++seen == 2 ? 7 : 0; });
      if (stop != (calls >= 2 ? 7 : 0) || seen != (calls >= 2 ? 2 : calls)) {
        fprintf(stderr, "a refusing callback: %d after %zu of %zu runs\n", stop, seen, calls);
        return 1;
      }
    } else {
      return 3;
    }
  }
  return 0;
}
