// pack_build_check.cpp — csrc/pack_build.hpp on its own, for a sanitizer build (test_pack_build_check.py compiles this with
// -fsanitize=address,undefined and runs it alone).  It reads a file of cases and prints one line per walk:
//   P <hex bytes>                                  a pack (numbered from 0 in order of appearance)
//   W <pack> <C> then C x (z consumed out_len status)   the walk over that pack with this table of candidates
// -> "<rc> <bad_offset> <bad_status> <n> <written>": the walk's answer, and what the idx writer made of the objects it found
// (0 when the walk failed; else the idx's length, after md::pack::read_index has read it back to the same entries).
// The pack and every array of the table live in heap blocks of exactly their length, so a read past an end is a finding.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pack_build.hpp"

template <class T>
static T *exact(const std::vector<T> &v) {
  T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

static void run(const std::vector<uint8_t> &bytes, const std::vector<uint64_t> &z, const std::vector<uint64_t> &consumed,
                const std::vector<uint64_t> &out_len, const std::vector<int32_t> &status) {
  uint8_t *pack = exact(bytes);
  uint64_t *pz = exact(z), *pc = exact(consumed), *po = exact(out_len);
  int32_t *ps = exact(status);
  md::pkb::Candidates c;
  c.C = z.size(), c.z = pz, c.consumed = pc, c.out_len = po, c.status = ps;
  md::pkb::Walk w;
  const int rc = md::pkb::walk(pack, bytes.size(), c, &w);
  size_t written = 0;
  if (rc == MD_OK) {
    const size_t n = w.off.size();
    std::vector<md_pack_index_entry> ent(n);
    for (size_t i = 0; i < n; i++) {  // made-up names that differ, in no order
      ent[i].offset = w.off[i], ent[i].crc32 = (uint32_t)w.inflated[i];
      memset(ent[i].name, 0, 20);
      const uint64_t key = w.off[i] * 0x9e3779b97f4a7c15ull;
      memcpy(ent[i].name, &key, 8);
      memcpy(ent[i].name + 8, &w.off[i], 8);
    }
    md_pack_index_entry *pe = exact(ent);
    size_t need = 0;
    if (md::pkb::write_index(pe, n, pack + bytes.size() - 20, nullptr, 0, &need) != MD_UNEXPECTED_END_OF_OUTPUT) exit(4);
    uint8_t *idx = (uint8_t *)malloc(need);
    if (md::pkb::write_index(pe, n, pack + bytes.size() - 20, idx, need, &written) != MD_OK || written != need) exit(4);
    md_pack_index_info info;
    md_pack_index_entry *back = (md_pack_index_entry *)malloc(n * sizeof(md_pack_index_entry) + 1);
    if (md::pack::read_index(idx, need, &info, back, n) != MD_OK || info.n != n) exit(5);
    for (size_t i = 0; i < n; i++) {  // every entry written is read back
      bool found = false;
      for (size_t k = 0; k < n && !found; k++) found = back[k].offset == ent[i].offset && back[k].crc32 == ent[i].crc32 && !memcmp(back[k].name, ent[i].name, 20);
      if (!found) exit(5);
    }
    free(back), free(idx), free(pe);
  }
  printf("%d %llu %d %zu %zu\n", rc, (unsigned long long)w.bad_offset, (int)w.bad_status, w.off.size(), written);
  free(pack), free(pz), free(pc), free(po), free(ps);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<std::vector<uint8_t>> packs;
  std::string line;
  int ch;
  while ((ch = fgetc(f)) != EOF) {
    if (ch != '\n') {
      line.push_back((char)ch);
      continue;
    }
    if (line.size() >= 2 && line[0] == 'P') {
      std::vector<uint8_t> b;
      for (size_t i = 2; i + 1 < line.size(); i += 2) b.push_back((uint8_t)strtoul(line.substr(i, 2).c_str(), nullptr, 16));
      if (b.size() < 32) return 3;  // (the call-level check is the caller's)
      packs.push_back(b);
    } else if (line.size() >= 2 && line[0] == 'W') {
      char *p = &line[1];
      const unsigned long long which = strtoull(p, &p, 10), C = strtoull(p, &p, 10);
      if (which >= packs.size()) return 3;
      std::vector<uint64_t> z(C), consumed(C), out_len(C);
      std::vector<int32_t> status(C);
      for (size_t k = 0; k < C; k++) {
        z[k] = strtoull(p, &p, 10), consumed[k] = strtoull(p, &p, 10), out_len[k] = strtoull(p, &p, 10);
        status[k] = (int32_t)strtol(p, &p, 10);
      }
      run(packs[which], z, consumed, out_len, status);
    }
    line.clear();
  }
  fclose(f);
  return 0;
}
