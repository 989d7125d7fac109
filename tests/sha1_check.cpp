// sha1_check.cpp — csrc/sha1_host.hpp on its own, for a sanitizer build (test_sha1_host_check.py compiles this with
// -fsanitize=address,undefined and runs it alone).  It reads a file of cases and prints one line of hex per case:
//   D <type> <hex bytes>   the digest of the bytes as an object of `type` (0: as they are), through sha1_object
//   S <hex bytes>          one digest per split point 0 .. n: the bytes fed to sha1_update in two pieces (n + 1 lines)
//   A <count>              the digest of `count` times 'a', fed in pieces of 1000 bytes
//   H <type> <size>        the header git_header writes, as hex, its length in front ("<len> <hex>")
// Every message is hashed from a heap block of exactly its length, so a read past the end is a finding.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sha1_host.hpp"

static void print_hex(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
  printf("\n");
}

static std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> b;
  for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return b;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  std::string line;
  int c;
  while ((c = fgetc(f)) != EOF) {
    if (c != '\n') {
      line.push_back((char)c);
      continue;
    }
    uint8_t digest[20];
    if (line.size() >= 3 && line[0] == 'D') {
      const uint32_t type = (uint32_t)(line[2] - '0');
      const std::vector<uint8_t> b = unhex(line.size() > 4 ? line.substr(4) : std::string());
      uint8_t *p = (uint8_t *)malloc(b.size() ? b.size() : 1);
      if (!b.empty()) memcpy(p, b.data(), b.size());
      md::sha::sha1_object(type, p, (uint32_t)b.size(), digest);
      free(p);
      print_hex(digest, 20);
    } else if (line.size() >= 2 && line[0] == 'S') {
      const std::vector<uint8_t> b = unhex(line.substr(2));
      for (size_t cut = 0; cut <= b.size(); cut++) {
        uint8_t *p = (uint8_t *)malloc(cut ? cut : 1), *q = (uint8_t *)malloc(b.size() - cut ? b.size() - cut : 1);
        if (cut) memcpy(p, b.data(), cut);
        if (b.size() - cut) memcpy(q, b.data() + cut, b.size() - cut);
        md::sha::Sha1 s;
        md::sha::sha1_init(&s);
        md::sha::sha1_update(&s, p, cut);
        md::sha::sha1_update(&s, q, b.size() - cut);
        md::sha::sha1_final(&s, digest);
        free(p);
        free(q);
        print_hex(digest, 20);
      }
    } else if (line.size() >= 3 && line[0] == 'A') {
      unsigned long count = strtoul(line.c_str() + 2, nullptr, 10);
      std::vector<uint8_t> piece(1000, (uint8_t)'a');
      md::sha::Sha1 s;
      md::sha::sha1_init(&s);
      for (; count >= 1000; count -= 1000) md::sha::sha1_update(&s, piece.data(), 1000);
      md::sha::sha1_update(&s, piece.data(), count);
      md::sha::sha1_final(&s, digest);
      print_hex(digest, 20);
    } else if (line.size() >= 5 && line[0] == 'H') {
      unsigned type = 0;
      unsigned long size = 0;
      if (sscanf(line.c_str() + 2, "%u %lu", &type, &size) != 2) return 3;
      uint32_t hw[md::sha::kHeaderWords];
      const uint32_t n = md::sha::git_header(type, (uint32_t)size, hw);
      uint8_t bytes[4 * md::sha::kHeaderWords];
      for (uint32_t i = 0; i < sizeof bytes; i++) bytes[i] = (uint8_t)(hw[i >> 2] >> (24 - 8 * (i & 3)));
      printf("%u ", n);
      print_hex(bytes, sizeof bytes);  // (all 20: what lies behind the header has to be zero)
    } else if (!line.empty()) {
      return 3;
    }
    line.clear();
  }
  fclose(f);
  return 0;
}
