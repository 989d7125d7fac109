/* oracle/de_deflate.c — TEST INFRASTRUCTURE ONLY (see oracle.h).
 *
 * CPU restatement of the reference's streaming DEFLATE compressor:
 *   De.Lz77   (zlib deflate_slow with a 4-byte multiplicative hash)  lib/de.ml:4013-4515
 *   De.Queue  (command ring)                                         lib/de.ml:2194-2328
 *   De.T      (Huffman tree construction)                            lib/de.ml:1828-2192
 *   De.Def    (block choice + LSB-first bit encoder)                 lib/de.ml:2354-3038
 *   drivers   Zl.Def.encode (lib/zl.ml:509-555), De.Higher.compress (lib/de.ml:4518-4553),
 *             the CLI/test driver (bin/decompress.ml:47-75, test/test.ml:1250-1266)
 *
 * PARITY: pinned only by the reference's encoder KATs (tests/golden/deflate_kat.json:
 * huffman_length_extra, flat, tree_0, tree_rfc5322) and by round trips through libz and
 * the inflate oracle.  Beyond those, byte-for-byte equality with the OCaml reference is
 * UNPINNED (the reference cannot be built in this image).  The parity hazards H1-H8 of
 * SURVEY.md 8(c) are restated deliberately (cumulative + mutated histograms, odd cost
 * formula, driver-dependent empty blocks, reads past the end of input).
 *
 * Window model (H7): the 64 KiB LZ77 window starts zeroed; whole input is supplied
 * in one `src` call followed by end-of-input, so the bytes the matcher reads beyond the
 * data are deterministic (zeros, or stale data of the previous 32 KiB).
 */
#include "oracle.h"
#include <stdlib.h>
#include <string.h>

#define MAX_BITS 15
#define L_CODES 286
#define D_CODES 30
#define BL_CODES 19
#define HEAP_SIZE (2 * L_CODES + 1) /* 573 */
#define LIT_FREQS (2 * L_CODES + 1)
#define DST_FREQS (2 * D_CODES + 1)

static const uint8_t zigzag[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
static const int base_length[32] = {0,  1,  2,  3,  4,  5,  6,   7,   8,  10, 12,
                                    14, 16, 20, 24, 28, 32, 40,  48,  56, 64, 80,
                                    96, 112, 128, 160, 192, 224, 255, 0,  0,  0};
static const int extra_lbits[32] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2,
                                    3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0, 0, 0, 0};
static const int extra_dbits[32] = {0, 0, 0, 0, 1, 1, 2,  2,  3,  3,  4,
                                    4, 5, 5, 6, 6, 7, 7,  8,  8,  9,  9,
                                    10, 10, 11, 11, 12, 12, 13, 13, 0, 0};
static const int base_dist[32] = {0,    1,    2,    3,    4,    6,     8,     12,
                                  16,   24,   32,   48,   64,   96,    128,   192,
                                  256,  384,  512,  768,  1024, 1536,  2048,  3072,
                                  4096, 6144, 8192, 12288, 16384, 24576, -1,  -1};

/* _length.(len) for len 3..258 (lib/de.ml:240-256) and _distance code (lib/de.ml:258-291):
 * computed from the base tables instead of transcribing the 259/512-entry arrays. */
static uint8_t length_code[259];
static uint8_t dist_code_lo[256], dist_code_hi[256];
static int tables_ready = 0;
static void init_tables(void) {
  if (tables_ready) return;
  for (int len = 0; len < 259; len++) {
    int c = 0;
    if (len >= 3) {
      int l = len - 3;
      if (l == 255) c = 28;
      else {
        for (c = 27; c > 0 && base_length[c] > l; c--) {}
      }
    }
    length_code[len] = (uint8_t)c;
  }
  for (int d = 0; d < 256; d++) { /* d = distance - 1 */
    int c;
    for (c = 29; c > 0 && base_dist[c] > d; c--) {}
    dist_code_lo[d] = (uint8_t)c;
  }
  for (int h = 0; h < 256; h++) { /* (distance-1) >> 7 */
    int d = h << 7;
    int c;
    for (c = 29; c > 0 && base_dist[c] > d; c--) {}
    dist_code_hi[h] = (uint8_t)c;
  }
  tables_ready = 1;
}
/* lib/de.ml:289-291 */
static int distance_code(int d1) { return d1 < 256 ? dist_code_lo[d1] : dist_code_hi[d1 >> 7]; }

/* static encode trees, lib/de.ml:373-420: (code reversed, len) */
static void static_lit(int sym, int *len, int *code) {
  int l, c;
  if (sym < 144) { l = 8; c = 0x30 + sym; }
  else if (sym < 256) { l = 9; c = 0x190 + (sym - 144); }
  else if (sym < 280) { l = 7; c = sym - 256; }
  else { l = 8; c = 0xc0 + (sym - 280); }
  int r = 0;
  for (int i = 0; i < l; i++) r |= ((c >> i) & 1) << (l - 1 - i);
  *len = l;
  *code = r;
}
static void static_dist(int sym, int *len, int *code) {
  int r = 0;
  for (int i = 0; i < 5; i++) r |= ((sym >> i) & 1) << (4 - i);
  *len = 5;
  *code = r;
}

/* ------------------------------------------------------------------------- */
/* De.T, lib/de.ml:1828-2192 */
typedef struct {
  int lengths[HEAP_SIZE]; /* T.tree.lengths: later patched by T.scan's 0xffff guard */
  int clen[HEAP_SIZE];    /* T.tree.tree (Lookup): code lengths as of T.make, used to encode */
  int codes[HEAP_SIZE];
  int max_code;
} tree_t;

typedef struct {
  int heap[HEAP_SIZE];
  int len, max;
} heap_t;

static int smaller(const int *freqs, int n, int m, const int *depth) {
  return freqs[n] < freqs[m] || (freqs[n] == freqs[m] && depth[n] <= depth[m]);
}
static void pqdownheap(const int *freqs, const int *depth, heap_t *h, int k) {
  int v = h->heap[k];
  int j = k << 1;
  while (j <= h->len) {
    if (j < h->len && smaller(freqs, h->heap[j + 1], h->heap[j], depth)) j++;
    if (smaller(freqs, v, h->heap[j], depth)) break;
    h->heap[k] = h->heap[j];
    k = j;
    j <<= 1;
  }
  h->heap[k] = v;
}
static unsigned reverse_code(unsigned code, int len) {
  unsigned res = 0;
  do {
    res |= code & 1;
    code >>= 1;
    res <<= 1;
  } while (--len > 0);
  return res >> 1;
}

/* T.make: `freqs` is the caller's live histogram and is MUTATED (H2):
 * pkzip forces freqs[0|1] = 1, internal node sums land in freqs[length ..]. */
static void tree_make(int length, int max_length, int *freqs, int *bl_count, tree_t *t) {
  heap_t h;
  int depth[HEAP_SIZE], dads[HEAP_SIZE];
  memset(&h, 0, sizeof h);
  h.max = HEAP_SIZE;
  memset(depth, 0, sizeof depth);
  memset(dads, 0, sizeof dads);
  memset(t->lengths, 0, sizeof t->lengths);
  int max_code = -1;
  for (int n = 0; n < length; n++) {
    if (freqs[n] != 0) {
      h.heap[++h.len] = n;
      max_code = n;
      depth[n] = 0;
    } else t->lengths[n] = 0;
  }
  while (h.len < 2) { /* pkzip, lib/de.ml:1863-1874 */
    int node = max_code < 2 ? ++max_code : 0;
    freqs[node] = 1;
    h.heap[++h.len] = node;
    depth[node] = 0;
  }
  for (int n = h.len / 2; n >= 1; n--) pqdownheap(freqs, depth, &h, n);
  int node = length;
  do {
    int n = h.heap[1];
    h.heap[1] = h.heap[h.len--];
    pqdownheap(freqs, depth, &h, 1);
    int m = h.heap[1];
    h.heap[--h.max] = n;
    h.heap[--h.max] = m;
    freqs[node] = freqs[n] + freqs[m];
    depth[node] = (depth[n] >= depth[m] ? depth[n] : depth[m]) + 1;
    dads[n] = dads[m] = node;
    h.heap[1] = node++;
    pqdownheap(freqs, depth, &h, 1);
  } while (h.len >= 2);
  h.heap[--h.max] = h.heap[1];
  /* generate_lengths, lib/de.ml:1952-2009 */
  t->lengths[h.heap[h.max]] = 0;
  int overflow = 0;
  for (int i = 0; i <= MAX_BITS; i++) bl_count[i] = 0;
  for (int hh = h.max + 1; hh < HEAP_SIZE; hh++) {
    int n = h.heap[hh];
    int bits = t->lengths[dads[n]] + 1;
    if (bits > max_length) {
      overflow++;
      bits = max_length;
    }
    t->lengths[n] = bits;
    if (n <= max_code) bl_count[bits]++;
  }
  if (overflow != 0) {
    do {
      int bits = max_length - 1;
      while (bl_count[bits] == 0) bits--;
      bl_count[bits]--;
      bl_count[bits + 1] += 2;
      bl_count[max_length]--;
      overflow -= 2;
    } while (overflow > 0);
    int hh = HEAP_SIZE;
    for (int bits = max_length; bits >= 1; bits--) {
      int n = bl_count[bits];
      while (n != 0) {
        int m = h.heap[--hh];
        if (m <= max_code) {
          if (t->lengths[m] != bits) t->lengths[m] = bits;
          n--;
        }
      }
    }
  }
  /* generate_codes, lib/de.ml:1926-1950 */
  int next_code[MAX_BITS + 1];
  unsigned code = 0;
  memset(t->codes, 0, sizeof t->codes);
  next_code[0] = 0;
  for (int bits = 1; bits <= MAX_BITS; bits++) {
    code = (code + (unsigned)bl_count[bits - 1]) << 1;
    next_code[bits] = (int)(code & 0xffff);
  }
  for (int n = 0; n <= max_code; n++) {
    int len = t->lengths[n];
    if (len > 0) t->codes[n] = (int)reverse_code((unsigned)next_code[len]++, len);
  }
  memcpy(t->clen, t->lengths, sizeof t->clen);
  t->max_code = max_code;
}

/* T.scan, lib/de.ml:2070-2117 */
static void tree_scan(int *lengths, int max_code, int *bl_freqs) {
  int prevlen = -1, nextlen = lengths[0], curlen, count = 0, max_count = 7, min_count = 4;
  if (nextlen == 0) { max_count = 138; min_count = 3; }
  lengths[max_code + 1] = 0xffff;
  for (int n = 0; n <= max_code; n++) {
    curlen = nextlen;
    nextlen = lengths[n + 1];
    if (++count < max_count && curlen == nextlen) continue;
    else if (count < min_count) bl_freqs[curlen] += count;
    else if (curlen != 0) {
      if (curlen != prevlen) bl_freqs[curlen]++;
      bl_freqs[16]++;
    } else if (count <= 10) bl_freqs[17]++;
    else bl_freqs[18]++;
    count = 0;
    prevlen = curlen;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    else if (curlen == nextlen) { max_count = 6; min_count = 3; }
    else { max_count = 7; min_count = 4; }
  }
}
/* T.symbols, lib/de.ml:2122-2191: entries are (len << 15) | code */
static int tree_symbols(int i, const int *lengths, int max_code, const tree_t *bl, int *out) {
#define BLSYM(c) ((bl->clen[c] << 15) | bl->codes[c])
  int prevlen = -1, nextlen = lengths[0], curlen, count = 0, max_count = 7, min_count = 4;
  if (nextlen == 0) { max_count = 138; min_count = 3; }
  for (int n = 0; n <= max_code; n++) {
    curlen = nextlen;
    nextlen = lengths[n + 1];
    if (++count < max_count && curlen == nextlen) continue;
    else if (count < min_count) {
      do out[i++] = BLSYM(curlen); while (--count != 0);
    } else if (curlen != 0) {
      if (curlen != prevlen) {
        out[i++] = BLSYM(curlen);
        count--;
      }
      out[i++] = BLSYM(16);
      out[i++] = (2 << 15) | (count - 3);
    } else if (count <= 10) {
      out[i++] = BLSYM(17);
      out[i++] = (3 << 15) | (count - 3);
    } else {
      out[i++] = BLSYM(18);
      out[i++] = (7 << 15) | (count - 11);
    }
    count = 0;
    prevlen = curlen;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    else if (curlen == nextlen) { max_count = 6; min_count = 3; }
    else { max_count = 7; min_count = 4; }
  }
  return i;
#undef BLSYM
}

/* Def.dynamic, lib/de.ml:2357-2407 */
typedef struct {
  tree_t ltree, dtree, bltree;
  int h_lit, h_dst, h_len;
  int symbols[L_CODES + D_CODES + 64];
  int nsymbols;
} dynamic_t;

static void dynamic_of_frequencies(int *literals, int *distances, dynamic_t *d) {
  int bl_count[MAX_BITS + 1];
  int bl_freqs[2 * BL_CODES + 1];
  tree_make(L_CODES, MAX_BITS, literals, bl_count, &d->ltree);
  tree_make(D_CODES, MAX_BITS, distances, bl_count, &d->dtree);
  memset(bl_freqs, 0, sizeof bl_freqs);
  tree_scan(d->ltree.lengths, d->ltree.max_code, bl_freqs);
  tree_scan(d->dtree.lengths, d->dtree.max_code, bl_freqs);
  tree_make(BL_CODES, 7, bl_freqs, bl_count, &d->bltree);
  int max_blindex = BL_CODES - 1;
  while (max_blindex >= 3 && d->bltree.lengths[zigzag[max_blindex]] == 0) max_blindex--;
  int i = tree_symbols(0, d->ltree.lengths, d->ltree.max_code, &d->bltree, d->symbols);
  i = tree_symbols(i, d->dtree.lengths, d->dtree.max_code, &d->bltree, d->symbols);
  d->nsymbols = i;
  d->h_lit = d->ltree.max_code + 1;
  d->h_dst = d->dtree.max_code + 1;
  d->h_len = max_blindex + 1;
}

/* lib/de.ml:2415-2441 — note the H3 quirk: `distances[i] + len` */
static long static_cost(const int *literals, const int *distances) {
  long bits = 0;
  for (int i = 0; i < L_CODES; i++)
    if (literals[i] != 0) {
      int l, c;
      static_lit(i, &l, &c);
      bits += (long)literals[i] * l;
    }
  for (int i = 0; i < D_CODES; i++)
    if (distances[i] != 0) bits += distances[i] + 5;
  return bits;
}
static long dynamic_cost(const dynamic_t *d, const int *literals, const int *distances) {
  long bits = 5 + 5 + 4 + d->h_len * 3;
  for (int i = 0; i < d->nsymbols; i++) bits += d->symbols[i] >> 15;
  for (int i = 0; i < L_CODES; i++)
    if (literals[i] != 0) bits += (long)literals[i] * d->ltree.lengths[i];
  for (int i = 0; i < D_CODES; i++)
    if (distances[i] != 0) bits += distances[i] + d->dtree.lengths[i];
  return bits;
}

enum { KIND_FLAT = 0, KIND_FIXED = 1, KIND_DYNAMIC = 2 };
typedef struct {
  int kind, last;
  dynamic_t dyn;
} block_t;

/* Def.block_of_frequencies, lib/de.ml:2443-2449 */
static void block_of_frequencies(int last, int *literals, int *distances, block_t *b) {
  dynamic_of_frequencies(literals, distances, &b->dyn);
  b->last = last;
  b->kind = dynamic_cost(&b->dyn, literals, distances) <= static_cost(literals, distances)
                ? KIND_DYNAMIC
                : KIND_FIXED;
}

/* ------------------------------------------------------------------------- */
/* De.Queue, lib/de.ml:2194-2328 */
typedef struct {
  int *buf;
  unsigned w, r, c;
} queue_t;
#define Q_EOB 256
#define Q_COPY 0x2000000
static unsigned q_size(const queue_t *q) { return q->w - q->r; }
static unsigned q_available(const queue_t *q) { return q->c - (q->w - q->r); }
static void q_push(queue_t *q, int v) { q->buf[q->w++ & (q->c - 1)] = v; }
static int q_peek(const queue_t *q) { return q->buf[q->r & (q->c - 1)]; }
static int q_end_with_eob(const queue_t *q) {
  return q_size(q) ? q->buf[(q->w - 1) & (q->c - 1)] == Q_EOB : 0;
}

/* growable output (the bitstream does not depend on how the output is chunked) */
typedef struct {
  uint8_t *p;
  size_t n, cap;
} out_t;
static void out_byte(out_t *o, unsigned b) {
  if (o->n == o->cap) {
    o->cap = o->cap ? o->cap * 2 : 4096;
    o->p = (uint8_t *)realloc(o->p, o->cap);
  }
  o->p[o->n++] = (uint8_t)b;
}

/* De.Def.encoder, lib/de.ml:2465-3038 */
enum { K_FIRST_ENTRY, K_ENCODE, K_BLOCK, K_FLAT_DONE };
enum { R_OK, R_BLOCK };
enum { V_AWAIT, V_FLUSH, V_BLOCK };
typedef struct {
  block_t blk;
  uint64_t hold;
  int bits;
  int flat, fmax;
  queue_t *q;
  out_t *o;
  int k;
  int bits_rem;
} enc_t;

static void put_bits(enc_t *e, unsigned v, int n) { /* c_bits / write: 16-bit stores */
  e->hold |= (uint64_t)v << e->bits;
  e->bits += n;
  while (e->bits >= 16) {
    out_byte(e->o, e->hold & 0xff);
    out_byte(e->o, (e->hold >> 8) & 0xff);
    e->hold >>= 16;
    e->bits -= 16;
  }
}
static void align_bits(enc_t *e) { /* flush_bits / pending_bits, lib/de.ml:2549-2564, 2635-2653 */
  if (e->bits > 8) {
    out_byte(e->o, e->hold & 0xff);
    out_byte(e->o, (e->hold >> 8) & 0xff);
  } else if (e->bits > 0) out_byte(e->o, e->hold & 0xff);
  e->hold = 0;
  e->bits = 0;
}
static void lit_code(const enc_t *e, int sym, int *len, int *code) {
  if (e->blk.kind == KIND_DYNAMIC) {
    *len = e->blk.dyn.ltree.clen[sym];
    *code = e->blk.dyn.ltree.codes[sym];
  } else static_lit(sym, len, code);
}
static void dst_code(const enc_t *e, int sym, int *len, int *code) {
  if (e->blk.kind == KIND_DYNAMIC) {
    *len = e->blk.dyn.dtree.clen[sym];
    *code = e->blk.dyn.dtree.codes[sym];
  } else static_dist(sym, len, code);
}
/* Def.exists, lib/de.ml:2451-2463 */
static int cmd_exists(const enc_t *e, int cmd) {
  if (e->blk.kind != KIND_DYNAMIC) return 1;
  if (cmd == Q_EOB) return 1;
  if (!(cmd & Q_COPY)) return e->blk.dyn.ltree.clen[cmd & 0xff] > 0;
  int off = cmd & 0xffff, len = (cmd >> 16) & 0x1ff;
  return e->blk.dyn.ltree.clen[257 + length_code[len + 3]] > 0 &&
         e->blk.dyn.dtree.clen[distance_code(off)] > 0;
}
static void emit_eob(enc_t *e) {
  int l, c;
  lit_code(e, 256, &l, &c);
  put_bits(e, (unsigned)c, l);
}
static int enc_write_flat(enc_t *e);
/* write, lib/de.ml:2708-2897 */
static int enc_write(enc_t *e) {
  while (q_size(e->q)) {
    int cmd = q_peek(e->q);
    if (!cmd_exists(e, cmd)) { /* Leave */
      emit_eob(e);
      e->k = K_BLOCK;
      return R_BLOCK;
    }
    e->q->r++;
    if (cmd == Q_EOB) { /* End */
      emit_eob(e);
      if (e->blk.last) {
        e->bits_rem = e->bits > 8 ? 16 - e->bits : e->bits > 0 ? 8 - e->bits : 0;
        align_bits(e);
        e->k = K_ENCODE;
        return R_OK;
      }
      e->k = K_BLOCK;
      return R_BLOCK;
    }
    int l, c;
    if (!(cmd & Q_COPY)) {
      lit_code(e, cmd, &l, &c);
      put_bits(e, (unsigned)c, l);
    } else {
      int off = cmd & 0xffff, len = (cmd >> 16) & 0x1ff;
      int code = length_code[len + 3];
      lit_code(e, code + 257, &l, &c);
      put_bits(e, (unsigned)c, l);
      put_bits(e, (unsigned)(len - base_length[code & 0x1f]), extra_lbits[code]);
      code = distance_code(off);
      dst_code(e, code, &l, &c);
      put_bits(e, (unsigned)c, l);
      put_bits(e, (unsigned)(off - base_dist[code]), extra_dbits[code & 0x1f]);
    }
  }
  e->k = K_ENCODE;
  return R_OK;
}
/* headers, lib/de.ml:2566-2633 */
static void emit_header(enc_t *e) {
  put_bits(e, e->blk.last ? 1 : 0, 1);
  if (e->blk.kind == KIND_FIXED) put_bits(e, 1, 2);
  else if (e->blk.kind == KIND_DYNAMIC) {
    const dynamic_t *d = &e->blk.dyn;
    put_bits(e, 2, 2);
    put_bits(e, (unsigned)(d->h_lit - 257), 5);
    put_bits(e, (unsigned)(d->h_dst - 1), 5);
    put_bits(e, (unsigned)(d->h_len - 4), 4);
    for (int r = 0; r < d->h_len; r++) put_bits(e, (unsigned)d->bltree.lengths[zigzag[r]], 3);
    for (int r = 0; r < d->nsymbols; r++) put_bits(e, (unsigned)(d->symbols[r] & 0x7fff), d->symbols[r] >> 15);
  } else {
    put_bits(e, 0, 2);
    align_bits(e);
    out_byte(e->o, e->fmax & 0xff);
    out_byte(e->o, (e->fmax >> 8) & 0xff);
    out_byte(e->o, (~e->fmax) & 0xff);
    out_byte(e->o, ((~e->fmax) >> 8) & 0xff);
    e->flat = 0;
  }
}
/* block, lib/de.ml:2657-2684 */
static int enc_block(enc_t *e, const block_t *b) {
  e->blk = *b;
  if (b->kind == KIND_FLAT) {
    if (q_end_with_eob(e->q)) e->q->w--;
    unsigned len = q_size(e->q);
    e->fmax = len < 0xffff ? (int)len : 0xffff;
    emit_header(e);
    e->k = K_ENCODE;
    return enc_write_flat(e);
  }
  emit_header(e);
  e->k = K_ENCODE;
  return enc_write(e);
}
/* write_flat, lib/de.ml:2927-2962 */
static int enc_write_flat(enc_t *e) {
  while (q_size(e->q) && e->flat < e->fmax) {
    int cmd = e->q->buf[e->q->r++ & (e->q->c - 1)];
    if (cmd != Q_EOB) {
      out_byte(e->o, cmd & 0xff);
      e->flat++;
    }
  }
  if (e->flat == e->fmax) {
    e->fmax = 0;
    if (e->blk.last) return R_OK;
    e->k = K_FLAT_DONE;
    return R_OK;
  }
  return R_OK;
}
/* force, lib/de.ml:2899-2924 */
static int enc_force(enc_t *e, const block_t *b) {
  if (e->blk.kind != KIND_FLAT) emit_eob(e);
  return enc_block(e, b);
}
/* Def.encode, lib/de.ml:2965-3038 */
static int enc_encode(enc_t *e, int v, const block_t *b) {
  switch (e->k) {
  case K_FIRST_ENTRY:
    if (v == V_BLOCK) return enc_block(e, b);
    /* `Flush / `Await with the initial {Fixed; last=false} block */
    if (e->blk.kind == KIND_FLAT) {
      if (q_end_with_eob(e->q)) e->q->w--;
      unsigned len = q_size(e->q);
      e->fmax = len < 0xffff ? (int)len : 0xffff;
    }
    emit_header(e);
    e->k = K_ENCODE;
    return enc_encode(e, v, b);
  case K_BLOCK:
    if (v == V_BLOCK) return enc_block(e, b);
    e->k = K_ENCODE;
    return enc_encode(e, v, b);
  case K_FLAT_DONE:
    if (v == V_BLOCK) return enc_block(e, b);
    e->k = K_BLOCK;
    return R_BLOCK;
  default:
    if (v == V_AWAIT) return R_OK;
    if (v == V_FLUSH) return e->blk.kind == KIND_FLAT ? enc_write_flat(e) : enc_write(e);
    return enc_force(e, b); /* `Block while a (non-last) block is open */
  }
}

/* ------------------------------------------------------------------------- */
/* De.Lz77, lib/de.ml:4013-4515 */
#define MIN_MATCH 3
#define MAX_MATCH 258
#define MIN_LOOKAHEAD (MAX_MATCH + MIN_MATCH + 1)
#define HASH_BITS 15
#define HASH_SIZE (1 << HASH_BITS)
#define TOO_FAR 4096
#define WBITS 15
#define WSIZE (1 << WBITS)
#define WMASK (WSIZE - 1)
#define MAX_DIST (WSIZE - MIN_LOOKAHEAD)

typedef struct {
  int max_chain, max_lazy, good_length, nice_length;
} lzcfg_t;
/* lib/de.ml:4030-4049: {good, lazy, nice, chain}; level 0 = Copy */
static const lzcfg_t lz_levels[10] = {
    {0, 0, 0, 0},         {4, 4, 4, 8},        {8, 5, 4, 16},         {32, 6, 4, 32},
    {16, 4, 4, 16},       {32, 16, 8, 32},     {128, 16, 8, 128},     {256, 32, 8, 128},
    {1024, 128, 32, 258}, {4096, 258, 32, 258}};

enum { LZ_FLUSH, LZ_END };
enum { LK_ENOUGH, LK_FILL };
typedef struct {
  int level;
  lzcfg_t cfg;
  const uint8_t *i;
  long i_pos, i_len; /* i_rem = i_len - i_pos + 1; EOI: i_len = LONG_MIN/2 */
  long n_total, piece; /* the whole input; how much of it one `Await brings */
  int lits[LIT_FREQS], dsts[DST_FREQS];
  uint8_t w[2 * WSIZE + 320]; /* +320: the matcher may look 260 bytes past the 64 KiB window at end of input */
  int lookahead, strstart;
  int prev[WSIZE], head[HASH_SIZE];
  int match_start, match_length, match_available, insert, prev_length, prev_match;
  queue_t *q;
  uint32_t crc;
  int k;
  int matcher; /* ORC_MATCHER_DE (De.Lz77) or ORC_MATCHER_LZ (lib/lz.ml) */
} lz_t;

static unsigned rd16(const uint8_t *p) { return p[0] | (p[1] << 8); }
static uint32_t rd32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
/* hash4, lib/de.ml:4067-4071 */
static unsigned hash4(const uint8_t *w, int off) {
  return (uint32_t)(rd32(w + off) * 0x9e3779b1u) >> (32 - HASH_BITS);
}
/* lib/lz.ml:153-155 update_hash (shift 5, 15 bits), rolled over the 3 bytes of a string:
 * insert_string (lib/lz.ml:297-304) updates with w[str + 2] a state that fill_window primed
 * with the two bytes at strstart (lib/lz.ml:399-401); every string that is inserted at all is
 * inserted right after its predecessor (skipped inserts only happen within the last
 * MIN_MATCH - 1 positions of the input), so the rolled value is this pure function. */
static unsigned hash3(const uint8_t *w, int off) {
  return (((unsigned)w[off] << 10) ^ ((unsigned)w[off + 1] << 5) ^ w[off + 2]) & (HASH_SIZE - 1);
}
static long lz_rem(const lz_t *s) { return s->i_len - s->i_pos + 1; }
static void lz_eoi(lz_t *s) {
  s->i_pos = 0;
  s->i_len = -(1L << 60);
}
/* The caller's answer to `Await: the next piece of the input (De.Lz77.src, lib/de.ml:4181-4188; `Manual refill :4200-4201), or the end of it.
 * orc_set_src_piece(p) makes the drivers below hand the input over p bytes at a time (0: all of it at once), which is
 * what decides how much fill_window finds each time it runs. */
static size_t g_src_piece = 0, g_src_first = 0;
void orc_set_src_piece(size_t piece) { g_src_piece = piece; }
/* ... with a FIRST piece of another size (0: like the others): what decides how far the window is written when
 * fill_window first slides it (lib/de.ml:4294-4312) - H7's door; the tail heads themselves: tests/lz77_cases.py, families E and F */
void orc_set_src_first_piece(size_t first) { g_src_first = first; }
static void lz_await(lz_t *s) {
  if (s->i_len + 1 < s->n_total) {
    long e = s->i_len + (long)s->piece;
    s->i_len = e < s->n_total - 1 ? e : s->n_total - 1;
  } else lz_eoi(s);
}
/* longest_match, lib/de.ml:4110-4174 */
static int longest_match(lz_t *s, int cur_match) {
  const uint8_t *w = s->w;
  int str_end = s->strstart + (MAX_MATCH - 1);
  int limit = s->strstart > MAX_DIST ? s->strstart - MAX_DIST : 0;
  int chain_length = s->prev_length >= s->cfg.good_length ? s->cfg.max_chain >> 2 : s->cfg.max_chain;
  unsigned scan_start = rd16(w + s->strstart);
  unsigned scan_end = rd16(w + s->strstart + s->prev_length - 1);
  int best_len = s->prev_length;
  for (;;) {
    int m = cur_match;
    if (rd16(w + m + best_len - 1) == scan_end && rd16(w + m) == scan_start) {
      int scan = s->strstart + 1;
      m++;
      while (scan < str_end && rd32(w + scan) == rd32(w + m)) { scan += 4; m += 4; }
      while (scan < str_end && rd16(w + scan) == rd16(w + m)) { scan += 2; m += 2; }
      while (scan < str_end && w[scan] == w[m]) { scan++; m++; }
      if (w[scan] == w[m]) scan++;
      int len = MAX_MATCH - 1 - (str_end - scan);
      if (len > best_len) {
        s->match_start = cur_match;
        best_len = len;
        if (len >= s->cfg.nice_length) break;
        scan_end = rd16(w + s->strstart + best_len - 1);
      }
    }
    cur_match = s->prev[cur_match & WMASK];
    chain_length--;
    if (!(cur_match > limit && chain_length != 0)) break;
  }
  return best_len <= s->lookahead ? best_len : s->lookahead;
}
static int insert_string(lz_t *s, int str) {
  unsigned h = s->matcher ? hash3(s->w, str) : hash4(s->w, str);
  int res = s->head[h];
  s->prev[str & WMASK] = res;
  s->head[h] = str;
  return res;
}
static int emit_tail(lz_t *s) { /* auto-EOB when one cell is left, lib/de.ml:4240-4243 */
  if (q_available(s->q) == 1) {
    q_push(s->q, Q_EOB);
    return 1;
  }
  return 0;
}
static int emit_match(lz_t *s, int off, int len) {
  q_push(s->q, ((len - 3) << 16) | (off - 1) | Q_COPY);
  s->lits[257 + length_code[len]]++;
  s->dsts[distance_code(off - 1)]++;
  return emit_tail(s);
}
static int emit_literal(lz_t *s, int chr) {
  q_push(s->q, chr);
  s->lits[chr]++;
  return emit_tail(s);
}
/* slide_hash, lib/de.ml:4268-4292 */
static void slide_hash(lz_t *s) {
  for (int p = 0; p < HASH_SIZE; p++) s->head[p] = s->head[p] >= WSIZE ? s->head[p] - WSIZE : 0;
  for (int p = 0; p < WSIZE; p++) s->prev[p] = s->prev[p] >= WSIZE ? s->prev[p] - WSIZE : 0;
}
/* deflate (one position), lib/de.ml:4351-4410.  Returns 1 on `Flush. */
static int lz_deflate(lz_t *s) {
  int hash_head = 0;
  if (s->lookahead >= MIN_MATCH) hash_head = insert_string(s, s->strstart);
  s->prev_length = s->match_length;
  s->prev_match = s->match_start;
  s->match_length = MIN_MATCH - 1;
  if (hash_head != 0 && s->prev_length < s->cfg.max_lazy && s->strstart - hash_head <= MAX_DIST) {
    int ml = longest_match(s, hash_head);
    if (ml <= 5 && ml == MIN_MATCH && s->strstart - s->match_start > TOO_FAR) s->match_length = MIN_MATCH - 1;
    else s->match_length = ml;
  }
  if (s->prev_length >= MIN_MATCH && s->match_length <= s->prev_length) {
    int max_insert = s->strstart + s->lookahead - MIN_MATCH;
    int flush = emit_match(s, s->strstart - 1 - s->prev_match, s->prev_length);
    s->lookahead -= s->prev_length - 1;
    s->prev_length -= 2;
    do {
      s->strstart++;
      if (s->strstart <= max_insert) insert_string(s, s->strstart);
    } while (--s->prev_length != 0);
    s->match_available = 0;
    s->match_length = MIN_MATCH - 1;
    s->strstart++;
    return flush;
  } else if (s->match_available) {
    int flush = emit_literal(s, s->w[s->strstart - 1]);
    s->strstart++;
    s->lookahead--;
    return flush;
  }
  s->match_available = 1;
  s->strstart++;
  s->lookahead--;
  return 0;
}
/* copy (level 0), lib/de.ml:4412-4423 */
static int lz_copy(lz_t *s) {
  int flush = q_available(s->q) <= 1;
  while (!flush && s->lookahead > 0) {
    flush = emit_literal(s, s->w[s->strstart]);
    s->strstart++;
    s->lookahead--;
  }
  return flush;
}
/* Lz77.compress: runs until `Flush or `End (input is complete, so `Await = EOI) */
static int lz_compress(lz_t *s) {
  for (;;) {
    if (s->k == LK_ENOUGH && s->lookahead >= MIN_LOOKAHEAD) goto work;
    /* fill_window, lib/de.ml:4294-4342 */
    {
      int more = 2 * WSIZE - s->lookahead - s->strstart;
      if (s->strstart >= WSIZE + MAX_DIST) {
        memcpy(s->w, s->w + WSIZE, (size_t)(WSIZE - more));
        s->match_start -= WSIZE;
        s->strstart -= WSIZE;
        slide_hash(s);
        more += WSIZE;
      }
      long rem = lz_rem(s);
      if (rem <= 0) {
        if (rem < 0) {
          if (s->lookahead > 0) goto work;
          /* trailing, lib/de.ml:4257-4266 */
          if (s->match_available) {
            int flush = emit_literal(s, s->w[s->strstart - 1]);
            s->insert = s->strstart < MIN_MATCH - 1 ? s->strstart : MIN_MATCH - 1;
            if (!flush && !s->matcher) q_push(s->q, Q_EOB);
          } else if (!s->matcher) q_push(s->q, Q_EOB); /* Lz.trailing pushes no EOB, lib/lz.ml:348-354 */
          return LZ_END;
        }
        lz_await(s); /* `Await -> the driver hands over the next piece, or signals end of input */
        s->k = LK_FILL;
        continue;
      }
      int len = more < rem ? more : (int)rem;
      memcpy(s->w + s->strstart + s->lookahead, s->i + s->i_pos, (size_t)len);
      s->crc = orc_adler32(s->crc, s->i + s->i_pos, (size_t)len);
      s->lookahead += len;
      s->i_pos += len;
      int brk = 0;
      if (s->lookahead + s->insert >= MIN_MATCH) {
        int str = s->strstart - s->insert, ins = s->insert;
        while (s->lookahead + ins >= MIN_MATCH && ins != 0) {
          unsigned h = s->matcher ? hash3(s->w, str) : hash4(s->w, str);
          s->prev[str & WMASK] = s->head[h];
          s->head[h] = str;
          str++;
          ins--;
          if (s->lookahead + ins < MIN_MATCH) {
            brk = 1;
            break;
          }
        }
        s->insert = ins;
      }
      if (!brk && s->lookahead < MIN_LOOKAHEAD && lz_rem(s) >= 0) {
        if (lz_rem(s) == 0) lz_await(s);
        s->k = LK_FILL;
        continue;
      }
    }
  work:
    s->k = LK_ENOUGH;
    if (s->level == 0 ? lz_copy(s) : lz_deflate(s)) return LZ_FLUSH;
  }
}

static lz_t *lz_new(int level, queue_t *q, const uint8_t *src, size_t n, int matcher) {
  lz_t *s = (lz_t *)calloc(1, sizeof *s);
  if (matcher && level < 4) level = 4; /* Lz.state: levels 0..4 are _4, no Copy mode (lib/lz.ml:535) */
  s->matcher = matcher;
  if (matcher) s->match_length = s->prev_length = MIN_MATCH - 1; /* lib/lz.ml:563-566 */
  s->level = level;
  s->cfg = lz_levels[level];
  s->i = src;
  s->i_pos = 0;
  s->n_total = (long)n;
  s->piece = g_src_piece && g_src_piece < n ? (long)g_src_piece : (long)n;
  s->i_len = (g_src_piece && g_src_first && g_src_first < n ? (long)g_src_first : s->piece) - 1;
  if (n == 0) lz_eoi(s);
  s->lits[256] = 1; /* make_literals, lib/de.ml:2333-2336 */
  s->q = q;
  s->crc = 1;
  s->k = LK_ENOUGH;
  return s;
}

/* ------------------------------------------------------------------------- */
/* drivers */
enum { DRV_ZL = 0, DRV_HIGHER = 1, DRV_CLI = 2 };

static void make_block(int driver, int dynamic, int last, lz_t *s, block_t *b) {
  if (driver == DRV_CLI) { /* always Dynamic (bin/decompress.ml:52-72); last block Fixed */
    b->last = last;
    if (last) b->kind = KIND_FIXED;
    else {
      dynamic_of_frequencies(s->lits, s->dsts, &b->dyn);
      b->kind = KIND_DYNAMIC;
    }
    return;
  }
  if (driver == DRV_ZL && s->level == 0) { /* Zl.Def.make_block, lib/zl.ml:501-507 */
    b->kind = KIND_FLAT;
    b->last = last;
    return;
  }
  if (driver == DRV_ZL && !dynamic) {
    b->kind = KIND_FIXED;
    b->last = last;
    return;
  }
  block_of_frequencies(last, s->lits, s->dsts, b);
}

/* Raw DEFLATE body produced by the reference's De.Lz77 + De.Def under `driver`.
 * Returns a malloc'ed buffer (*out_len bytes); *adler = Adler-32 of the input. */
uint8_t *orc_deflate_raw(const uint8_t *src, size_t n, int level, int queue_len, int driver,
                         int dynamic, size_t *out_len, uint32_t *adler) {
  return orc_deflate_raw_m(src, n, level, queue_len, driver, dynamic, ORC_MATCHER_DE, out_len, adler);
}

/* Same with the match finder chosen: ORC_MATCHER_LZ = lib/lz.ml (`Lz.state` / `Lz.compress`,
 * SURVEY 8(a) D12) feeding De.Def under the same drivers.  lib/lz.ml has no caller and no test
 * in the reference; the driver conventions assumed here: the driver pushes the end-of-block
 * command at `End when the queue does not already end with one (Lz.trailing does not), and
 * there is no Flat mode (Lz has no level-0 copy). */
uint8_t *orc_deflate_raw_m(const uint8_t *src, size_t n, int level, int queue_len, int driver,
                           int dynamic, int matcher, size_t *out_len, uint32_t *adler) {
  init_tables();
  if (level < 0 || level > 9 || queue_len < 4 || (queue_len & (queue_len - 1))) return NULL;
  queue_t q = {(int *)calloc((size_t)queue_len, sizeof(int)), 0, 0, (unsigned)queue_len};
  out_t o = {NULL, 0, 0};
  lz_t *s = lz_new(driver == DRV_HIGHER ? 4 : level, &q, src, n, matcher); /* H6: De.Higher has no ?level */
  enc_t e;
  memset(&e, 0, sizeof e);
  e.blk.kind = KIND_FIXED;
  e.q = &q;
  e.o = &o;
  e.k = K_FIRST_ENTRY;
  block_t *b = (block_t *)calloc(1, sizeof *b);
  int first = 1;
  for (;;) {
    int r = lz_compress(s);
    int rc;
    if (r == LZ_FLUSH) {
      if (driver == DRV_ZL) {
        /* lib/zl.ml:530-533: first `Flush sends a `Block, later ones `Flush */
        if (first) {
          first = 0;
          make_block(driver, dynamic, 0, s, b);
          rc = enc_encode(&e, V_BLOCK, b);
        } else rc = enc_encode(&e, V_FLUSH, NULL);
      } else {
        /* lib/de.ml:4532, bin/decompress.ml:56-60: every `Flush sends a fresh block */
        make_block(driver, dynamic, 0, s, b);
        rc = enc_encode(&e, V_BLOCK, b);
      }
      /* `Block reply: Zl.Def and De.Higher send a block again (lib/zl.ml:542-544,
       * lib/de.ml:4541); the CLI driver just goes on (bin/decompress.ml:70-72) */
      while (rc == R_BLOCK && driver != DRV_CLI) {
        make_block(driver, dynamic, 0, s, b);
        rc = enc_encode(&e, V_BLOCK, b);
      }
    } else {
      if (driver == DRV_CLI) { /* bin/decompress.ml:67: extra EOB */
        if (q_available(&q) == 0) { /* Queue.push_exn raises Queue.Full (lib/de.ml:2211, :2231-2236) */
          free(q.buf);
          free(s);
          free(b);
          free(o.p);
          *out_len = 0;
          return NULL;
        }
        q_push(&q, Q_EOB);
      }
      else if (matcher && !q_end_with_eob(&q)) q_push(&q, Q_EOB);
      make_block(driver, dynamic, 1, s, b);
      rc = enc_encode(&e, V_BLOCK, b);
      (void)rc;
      break;
    }
  }
  *adler = s->crc;
  *out_len = o.n;
  free(q.buf);
  free(s);
  free(b);
  if (!o.p) o.p = (uint8_t *)malloc(1);
  return o.p;
}

/* Zl.Def (lib/zl.ml:509-555): header 0x78xx, body, Adler-32 BE. */
uint8_t *orc_zl_deflate(const uint8_t *src, size_t n, int level, int queue_len, int dynamic,
                        size_t *out_len) {
  size_t blen;
  uint32_t adler;
  uint8_t *body = orc_deflate_raw(src, n, level, queue_len, DRV_ZL, dynamic, &blen, &adler);
  if (!body) return NULL;
  uint8_t *out = (uint8_t *)malloc(blen + 6);
  /* header, lib/zl.ml:512-517, FLEVEL map lib/zl.ml:580-581 */
  int flevel = level == 0 ? 0 : level <= 5 ? 1 : level == 6 ? 2 : 3;
  unsigned header = (8 + ((15 - 8) << 4)) << 8;
  header |= (unsigned)flevel << 6;
  header += 31 - (header % 31);
  out[0] = (uint8_t)(header >> 8);
  out[1] = (uint8_t)header;
  memcpy(out + 2, body, blen);
  out[2 + blen] = (uint8_t)(adler >> 24);
  out[3 + blen] = (uint8_t)(adler >> 16);
  out[4 + blen] = (uint8_t)(adler >> 8);
  out[5 + blen] = (uint8_t)adler;
  free(body);
  *out_len = blen + 6;
  return out;
}

void orc_free(void *p) { free(p); }

/* ------------------------------------------------------------------------- */
/* KAT helpers (tests/golden/deflate_kat.json) */

/* T.make on a histogram: fills lengths[n]/codes[n] for n < length; returns max_code. */
int orc_tree_make(int length, int max_length, int *freqs, int nfreqs, int *lengths, int *codes) {
  init_tables();
  int f[HEAP_SIZE];
  memset(f, 0, sizeof f);
  for (int i = 0; i < nfreqs && i < HEAP_SIZE; i++) f[i] = freqs[i];
  int bl_count[MAX_BITS + 1];
  tree_t *t = (tree_t *)calloc(1, sizeof *t);
  tree_make(length, max_length, f, bl_count, t);
  for (int i = 0; i < length; i++) {
    lengths[i] = t->lengths[i];
    codes[i] = t->codes[i];
  }
  for (int i = 0; i < nfreqs && i < HEAP_SIZE; i++) freqs[i] = f[i];
  int mc = t->max_code;
  free(t);
  return mc;
}

/* Encode a command list in ONE last block, like test/test.ml `encode` (lib/de.ml: Def.encode
 * (`Block {kind; last=true}) then `Flush).  kind: 0 Flat, 1 Fixed, 2 Dynamic built from the
 * commands' own frequencies (encode_dynamic, test/test.ml:84-95).
 * cmds: literal = byte value, End = 256, copy = ((len-3)<<16)|(off-1)|0x2000000. */
uint8_t *orc_encode_cmds(const int *cmds, int ncmds, int kind, size_t *out_len) {
  init_tables();
  unsigned cap = 4;
  while (cap < (unsigned)ncmds + 1) cap <<= 1;
  queue_t q = {(int *)calloc(cap, sizeof(int)), 0, 0, cap};
  int lits[LIT_FREQS], dsts[DST_FREQS];
  memset(lits, 0, sizeof lits);
  memset(dsts, 0, sizeof dsts);
  lits[256] = 1;
  for (int i = 0; i < ncmds; i++) {
    q_push(&q, cmds[i]);
    if (cmds[i] == Q_EOB) continue;
    if (cmds[i] & Q_COPY) {
      lits[257 + length_code[((cmds[i] >> 16) & 0x1ff) + 3]]++;
      dsts[distance_code(cmds[i] & 0xffff)]++;
    } else lits[cmds[i] & 0xff]++;
  }
  out_t o = {NULL, 0, 0};
  enc_t e;
  memset(&e, 0, sizeof e);
  e.blk.kind = KIND_FIXED;
  e.q = &q;
  e.o = &o;
  e.k = K_FIRST_ENTRY;
  block_t *b = (block_t *)calloc(1, sizeof *b);
  b->kind = kind;
  b->last = 1;
  if (kind == KIND_DYNAMIC) dynamic_of_frequencies(lits, dsts, &b->dyn);
  int rc = enc_encode(&e, V_BLOCK, b);
  if (rc == R_OK) enc_encode(&e, V_FLUSH, NULL);
  free(q.buf);
  free(b);
  *out_len = o.n;
  if (!o.p) o.p = (uint8_t *)malloc(1);
  return o.p;
}

/* De.Def.encode (lib/de.ml:2965-3038) driven step by step, the way test/test_ns.ml:388-615 and test/test.ml:533-767
 * drive it: one encoder over a queue of queue_len cells and a `Buffer.  ops (32-bit words):
 *   1 n c1..cn   Queue.push_exn of n commands      2 kind last  encode (`Block {kind; last}); kind 2 = Dynamic
 *   3            encode `Flush                                    (dynamic_of_frequencies of the live histograms)
 *   4 chr / 5 len / 6 dist   succ_literal / succ_length / succ_distance (lib/de.ml:2339-2351)
 *   7            make_literals () / make_distances ()             8  Queue.reset
 * rcs[k] = 0 `Ok / 1 `Block of the k-th encode.  NULL = Queue.Full or a malformed list. */
uint8_t *orc_def_script(const int *ops, int nops, int queue_len, int *rcs, int max_rcs, int *nrcs, size_t *out_len) {
  init_tables();
  queue_t q = {(int *)calloc((size_t)queue_len, sizeof(int)), 0, 0, (unsigned)queue_len};
  int lits[LIT_FREQS], dsts[DST_FREQS];
  memset(lits, 0, sizeof lits);
  memset(dsts, 0, sizeof dsts);
  lits[256] = 1;
  out_t o = {NULL, 0, 0};
  enc_t e;
  memset(&e, 0, sizeof e);
  e.blk.kind = KIND_FIXED;
  e.q = &q;
  e.o = &o;
  e.k = K_FIRST_ENTRY;
  block_t *b = (block_t *)calloc(1, sizeof *b);
  int n = 0, bad = 0;
  for (int i = 0; i < nops && !bad;) {
    int op = ops[i++], rc = -1;
    switch (op) {
    case 1: {
      if (i >= nops || ops[i] < 0 || ops[i] > nops - i - 1) { bad = 1; break; }
      int k = ops[i++];
      for (; k > 0 && !bad; k--) {
        if (q_available(&q) == 0) bad = 1; /* Queue.Full */
        else q_push(&q, ops[i++]);
      }
      break;
    }
    case 2:
      if (i + 1 >= nops || ops[i] < 0 || ops[i] > 2) { bad = 1; break; }
      b->kind = ops[i++];
      b->last = ops[i++] ? 1 : 0;
      if (b->kind == KIND_DYNAMIC) dynamic_of_frequencies(lits, dsts, &b->dyn);
      rc = enc_encode(&e, V_BLOCK, b);
      break;
    case 3: rc = enc_encode(&e, V_FLUSH, NULL); break;
    case 4: if (i >= nops) bad = 1; else lits[ops[i++] & 0xff]++; break;
    case 5: if (i >= nops || ops[i] < 3 || ops[i] > 258) bad = 1; else lits[257 + length_code[ops[i++]]]++; break;
    case 6: if (i >= nops || ops[i] < 1 || ops[i] > 32768) bad = 1; else dsts[distance_code(ops[i++] - 1)]++; break;
    case 7:
      memset(lits, 0, sizeof lits);
      memset(dsts, 0, sizeof dsts);
      lits[256] = 1;
      break;
    case 8: q.w = q.r = 0; break;
    default: bad = 1;
    }
    if (rc >= 0) {
      if (n < max_rcs) rcs[n] = rc == R_BLOCK ? 1 : 0;
      n++;
    }
  }
  free(q.buf);
  free(b);
  *nrcs = n;
  *out_len = o.n;
  if (bad) {
    free(o.p);
    return NULL;
  }
  if (!o.p) o.p = (uint8_t *)malloc(1);
  return o.p;
}

/* De.Lz77 alone (test/test.ml:798-813): the commands of every queue fill in order — what a caller of
 * De.Lz77.compress takes out of the queue at each `Flush and at `End (lib/de.mli:453-524) — and the cumulative
 * literals / distances histograms.  Returns the number of commands (they are stored while they fit in `max`). */
int orc_lz77_cmds_ex(const uint8_t *src, size_t n, int level, int queue_len, int matcher, int *out, int max, int *lits286,
                     int *dsts30) {
  init_tables();
  queue_t q = {(int *)calloc((size_t)queue_len, sizeof(int)), 0, 0, (unsigned)queue_len};
  lz_t *s = lz_new(level, &q, src, n, matcher);
  int cnt = 0;
  for (;;) {
    int r = lz_compress(s);
    while (q_size(&q)) {
      int c = q.buf[q.r++ & (q.c - 1)];
      if (cnt < max) out[cnt] = c;
      cnt++;
    }
    if (r == LZ_END) break;
  }
  if (lits286) memcpy(lits286, s->lits, 286 * sizeof(int));
  if (dsts30) memcpy(dsts30, s->dsts, 30 * sizeof(int));
  free(q.buf);
  free(s);
  return cnt;
}

/* De.Lz77 alone (test/test.ml:798-813): the command list of an input that fits one
 * queue fill.  Returns the number of commands (including the final End = 256), or -1
 * when the queue flushed before the end. */
int orc_lz77_cmds(const uint8_t *src, size_t n, int level, int queue_len, int *out, int max) {
  init_tables();
  queue_t q = {(int *)calloc((size_t)queue_len, sizeof(int)), 0, 0, (unsigned)queue_len};
  lz_t *s = lz_new(level, &q, src, n, ORC_MATCHER_DE);
  int r = lz_compress(s);
  int cnt = -1;
  if (r == LZ_END) {
    cnt = 0;
    while (q_size(&q) && cnt < max) out[cnt++] = q.buf[q.r++ & (q.c - 1)];
  }
  free(q.buf);
  free(s);
  return cnt;
}
