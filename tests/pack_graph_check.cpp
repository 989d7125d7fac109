// pack_graph_check.cpp — csrc/pack_graph.hpp on the host, for tests/test_pack_graph_check.py: the parse functions the link
// kernels run, over objects given as hex, built with AddressSanitizer and UBSan (every object stands in a heap block of
// exactly its size, so a read past its end is seen).  No device, nothing preloaded.
//
//   input   one object a line: "<type 1|2|4> <hex of its bytes, or - for none>"
//   output  one line each: "bad", or its edges in order, " <kind>:<40 hex of the name>" each (a tag's: ":<type>" behind it),
//           behind their number and the bound pack_graph.hpp gives for the object's size
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <string>

#include "pack_graph.hpp"

namespace pg = md::pg;

static std::string hex_of(const uint8_t *name) {
  static const char *digits = "0123456789abcdef";
  std::string s;
  for (int k = 0; k < 20; k++) s += digits[name[k] >> 4], s += digits[name[k] & 15];
  return s;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    const uint32_t type = (uint32_t)(line[0] - '0');
    const std::string hex = line.substr(2) == "-" ? "" : line.substr(2);
    const size_t size = hex.size() / 2;
    uint8_t *a = new uint8_t[size];
    for (size_t k = 0; k < size; k++) a[k] = (uint8_t)(pg::hex_digit((uint8_t)hex[2 * k]) << 4 | pg::hex_digit((uint8_t)hex[2 * k + 1]));
    std::string out;
    uint64_t count = 0;
    bool ok = true;
    if (type == 2) {
      ok = pg::tree_walk(a, size, [&](uint64_t pos, uint32_t kind, const uint8_t *name) {
        if (pos != count++) abort();
        out += " " + std::to_string(kind) + ":" + hex_of(name);
      });
    } else if (type == 1) {
      ok = pg::commit_walk(a, size, [&](uint64_t pos, uint32_t kind, const uint8_t *h) {
        if (pos != count++) abort();
        uint8_t name[20];
        for (uint32_t k = 0; k < 20; k++) name[k] = (uint8_t)pg::hex_byte(h, k);
        out += " " + std::to_string(kind) + ":" + hex_of(name);
      });
    } else {
      const uint32_t t = pg::tag_target_type(a, size);
      ok = t != 0;
      if (ok) {
        uint8_t name[20];
        for (uint32_t k = 0; k < 20; k++) name[k] = (uint8_t)pg::hex_byte(a + 7, k);
        out += " " + std::to_string(pg::kTagTarget) + ":" + hex_of(name) + ":" + std::to_string(t);
        count = 1;
      }
    }
    if (ok && count > pg::edge_bound(type, size)) abort();  // (a slot of the device holds edge_bound edges)
    if (ok) std::cout << count << out << "\n";
    else std::cout << "bad\n";
    delete[] a;
  }
  return 0;
}
