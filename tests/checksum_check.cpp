// checksum_check.cpp — the host checksums of csrc/host_util.hpp on their own, for a sanitizer build
// (test_checksum_host_check.py compiles this with -fsanitize=address,undefined and runs it alone).  It takes a file of cases
// and a file of bytes the cases point into, and prints one line of hex per answer:
//   A <seed> <off> <len> <shift>          md::adler32_update(seed, bytes[off, off + len))
//   P <seed> <off> <len> <piece>          the same chained over pieces of `piece` bytes, every piece a block of its own
//   C <crc> <off> <len> <shift>           md::crc32_update(crc, bytes[off, off + len))
//   Q <crc> <off> <len> <piece>           the same chained over pieces
//   S <off> <len>                         one line per split point 0 .. len: crc32_update over the two parts, chained
//   Z <crc> <n>                           crc32_update from `crc` chained over n zero bytes in blocks of 65536
//   K <crc_a> <crc_b> <len_b>             md::crc32_concat
//   J <crc_a> <z1> <n1> <z2> <n2>         crc32_concat(crc32_concat(crc_a, z1, n1), z2, n2)
//   W <z> <n> <k>                         k lines: z = crc32_concat(z, z, n), n = 2 n - the CRC of a zero run, doubled
// Numbers are hexadecimal.  Every message is read from a heap block that ends with its last byte (and starts `shift` bytes
// into the block, for the 8-byte loads of crc32_update), so a read past the end is a finding.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host_util.hpp"

namespace {
struct Block {  // bytes[off, off + len) at p, the block's last `len` bytes
  uint8_t *base, *p;
  Block(const std::vector<uint8_t> &bytes, size_t off, size_t len, size_t shift) {
    base = (uint8_t *)malloc(shift + len ? shift + len : 1);
    p = base + shift;
    if (len) memcpy(p, bytes.data() + off, len);
  }
  ~Block() { free(base); }
};
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::vector<uint8_t> bytes;
  {
    FILE *g = fopen(argv[2], "rb");
    if (!g) return 2;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, g)) > 0) bytes.insert(bytes.end(), buf, buf + k);
    fclose(g);
  }
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  char line[256];
  while (fgets(line, sizeof line, f)) {
    unsigned long long v[5] = {0, 0, 0, 0, 0};
    const int got = sscanf(line + 1, "%llx %llx %llx %llx %llx", &v[0], &v[1], &v[2], &v[3], &v[4]);
    const char op = line[0];
    if (op == '\n') continue;
    const bool ranged = op == 'A' || op == 'P' || op == 'C' || op == 'Q';
    if (ranged && (got != 4 || v[1] > bytes.size() || v[2] > bytes.size() - v[1])) return 3;
    if (op == 'A' || op == 'C') {
      const Block b(bytes, v[1], v[2], v[3]);
      printf("%08x\n", op == 'A' ? md::adler32_update((uint32_t)v[0], b.p, v[2]) : md::crc32_update((uint32_t)v[0], b.p, v[2]));
    } else if (op == 'P' || op == 'Q') {
      if (v[3] == 0) return 3;
      uint32_t s = (uint32_t)v[0];
      for (size_t at = 0; at < v[2]; at += v[3]) {
        const size_t k = v[2] - at < v[3] ? v[2] - at : v[3];
        const Block b(bytes, v[1] + at, k, 0);
        s = op == 'P' ? md::adler32_update(s, b.p, k) : md::crc32_update(s, b.p, k);
      }
      printf("%08x\n", s);
    } else if (op == 'S') {
      if (got != 2 || v[0] > bytes.size() || v[1] > bytes.size() - v[0]) return 3;
      for (size_t cut = 0; cut <= v[1]; cut++) {
        const Block lo(bytes, v[0], cut, 0), hi(bytes, v[0] + cut, v[1] - cut, 0);
        printf("%08x\n", md::crc32_update(md::crc32_update(0, lo.p, cut), hi.p, v[1] - cut));
      }
    } else if (op == 'Z') {
      if (got != 2) return 3;
      uint8_t *z = (uint8_t *)calloc(65536, 1);
      uint32_t c = (uint32_t)v[0];
      for (unsigned long long left = v[1]; left;) {
        const size_t k = left < 65536 ? (size_t)left : 65536;
        c = md::crc32_update(c, z + (65536 - k), k);  // (a shorter block ends where the allocation ends)
        left -= k;
      }
      free(z);
      printf("%08x\n", c);
    } else if (op == 'K') {
      if (got != 3) return 3;
      printf("%08x\n", md::crc32_concat((uint32_t)v[0], (uint32_t)v[1], v[2]));
    } else if (op == 'J') {
      if (got != 5) return 3;
      printf("%08x\n", md::crc32_concat(md::crc32_concat((uint32_t)v[0], (uint32_t)v[1], v[2]), (uint32_t)v[3], v[4]));
    } else if (op == 'W') {
      if (got != 3) return 3;
      uint32_t z = (uint32_t)v[0];
      uint64_t n = v[1];
      for (unsigned long long k = 0; k < v[2]; k++) {
        z = md::crc32_concat(z, z, n);
        n *= 2;
        printf("%08x\n", z);
      }
    } else {
      return 3;
    }
  }
  fclose(f);
  return 0;
}
