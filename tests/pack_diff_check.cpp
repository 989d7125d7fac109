// pack_diff_check.cpp — csrc/pack_diff.hpp on the host, for tests/test_pack_diff_check.py: the canonical mode, the key compare,
// the search by key and the classification that the diff kernels run, over pairs of trees given as hex, built with
// AddressSanitizer and UBSan (every tree stands in a heap block of exactly its size, so a read past its end is seen).  No
// device, nothing preloaded.
//
//   input   one pair a line: "<hex of A's bytes, or - for none> <hex of B's bytes, or ->"
//   output  one line each: "bad" when a side cannot be walked or is not sorted, else the number of records and, in the
//           records' order, " <kind>:<a's mode, octal>:<b's mode>:<hex of the name>" each
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "pack_diff.hpp"

namespace pd = md::pd;
namespace pg = md::pg;

struct Tree {
  uint8_t *a = nullptr;
  size_t size = 0;
  std::vector<pd::Entry> rows;
  bool ok = false;
};

static void load(const std::string &hex, Tree *t) {
  t->size = hex == "-" ? 0 : hex.size() / 2;
  t->a = new uint8_t[t->size];
  for (size_t k = 0; k < t->size; k++) t->a[k] = (uint8_t)(pg::hex_digit((uint8_t)hex[2 * k]) << 4 | pg::hex_digit((uint8_t)hex[2 * k + 1]));
  uint32_t start = 0;
  t->ok = pg::tree_walk(t->a, t->size, [&](uint64_t, uint32_t, const uint8_t *name) {
    const uint32_t nul = (uint32_t)(name - t->a) - 1;
    const uint32_t mode = pd::entry_mode(t->a, start, nul);
    if (mode == 0) abort();  // (tree_walk took the entry)
    t->rows.push_back(pd::Entry{start, pd::entry_name(t->a, start), nul, mode});
    start = nul + 21;
  });
  if (t->ok && t->rows.size() > t->size / pg::kMinEntry) abort();  // (a slot of the device holds size / 24 rows)
  for (size_t e = 0; t->ok && e + 1 < t->rows.size(); e++) t->ok = pd::key_compare(t->a, t->rows[e], t->a, t->rows[e + 1]) < 0;
}

static std::string record(uint32_t kind, uint32_t ma, uint32_t mb, const Tree &t, const pd::Entry &e) {
  static const char *digits = "0123456789abcdef";
  char head[64];
  snprintf(head, sizeof head, " %c:%o:%o:", (int)kind, ma, mb);
  std::string s = head;
  for (uint32_t k = e.name; k < e.nul; k++) s += digits[t.a[k] >> 4], s += digits[t.a[k] & 15];
  return s;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string ha, hb;
  while (in >> ha >> hb) {
    Tree A, B;
    load(ha, &A), load(hb, &B);
    if (!A.ok || !B.ok) {
      std::cout << "bad\n";
    } else {
      std::string out;
      size_t count = 0;
      const uint32_t na = (uint32_t)A.rows.size(), nb = (uint32_t)B.rows.size();
      for (uint32_t i = 0; i < na; i++) {
        const pd::Entry &x = A.rows[i];
        const uint32_t j = pd::find_key(A.a, x, B.a, [&](uint32_t k) { return B.rows[k]; }, nb);
        const bool found = j != pd::kNone;
        const uint32_t mb = found ? B.rows[j].mode : 0;
        const uint32_t kind = pd::classify(found, x.mode, mb, found && pd::same_name20(A.a + x.nul + 1, B.a + B.rows[j].nul + 1));
        if (kind) out += record(kind, x.mode, mb, A, x), count++;
      }
      for (uint32_t i = 0; i < nb; i++) {
        const pd::Entry &y = B.rows[i];
        if (pd::find_key(B.a, y, A.a, [&](uint32_t k) { return A.rows[k]; }, na) == pd::kNone) out += record('A', 0, y.mode, B, y), count++;
      }
      std::cout << count << out << "\n";
    }
    delete[] A.a;
    delete[] B.a;
  }
  return 0;
}
