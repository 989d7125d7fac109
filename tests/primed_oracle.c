/* tests/primed_oracle.c - TEST INFRASTRUCTURE ONLY: the body of one PRIMED span (mdeflate.h) from the oracle's own
 * matcher and encoder.  tests/primed_spans_model.py compiles it into a temporary directory when it is first used.
 *
 * It includes oracle/de_deflate.c as it stands and adds one function: the oracle's lz_t is built, the matcher walks positions
 * [0, first) of the stream with the oracle's own fill and insert steps - at each position it inserts the position if
 * lookahead >= MIN_MATCH, then strstart += 1, lookahead -= 1; it never calls longest_match and emits nothing - and then
 * the drivers' loop of orc_deflate_raw_m runs, restated here (that function builds its own lz_t, so it cannot be called).
 * With first = 0 the result is orc_deflate_raw_m's, which tests/test_primed_spans_model.py holds it to. */
#define orc_adler32 prm_adler32 /* (de_inflate.c has the oracle's; this file stands alone) */
#include "../oracle/de_deflate.c"

uint32_t prm_adler32(uint32_t adler, const uint8_t *buf, size_t len) {
  uint32_t a = adler & 0xffff, b = adler >> 16;
  for (size_t i = 0; i < len; i++) {
    a = (a + buf[i]) % 65521u;
    b = (b + a) % 65521u;
  }
  return (b << 16) | a;
}

/* The walk over the prefix.  first <= WSIZE, so the window does not slide here (that takes strstart >= WSIZE + MAX_DIST);
 * s->insert is 0 until `trailing` sets it, so fill_window's re-insertion loop has nothing to do.  The rest is
 * lz_compress's own sequence: fill when the look-ahead runs low, `Await when the input buffer is empty. */
static void prime_walk(lz_t *s, int first) {
  while (s->strstart < first) {
    if (!(s->k == LK_ENOUGH && s->lookahead >= MIN_LOOKAHEAD)) {
      int more = 2 * WSIZE - s->lookahead - s->strstart;
      long rem = lz_rem(s);
      if (rem == 0) {
        lz_await(s);
        s->k = LK_FILL;
        continue;
      }
      if (rem > 0) {
        int len = more < rem ? more : (int)rem;
        memcpy(s->w + s->strstart + s->lookahead, s->i + s->i_pos, (size_t)len);
        s->lookahead += len;
        s->i_pos += len;
        if (s->lookahead < MIN_LOOKAHEAD && lz_rem(s) >= 0) {
          if (lz_rem(s) == 0) lz_await(s);
          s->k = LK_FILL;
          continue;
        }
      }
      /* rem < 0, the end of the input: strstart < first <= n, so lookahead > 0 and the matcher works */
    }
    s->k = LK_ENOUGH;
    if (s->lookahead >= MIN_MATCH) insert_string(s, s->strstart);
    s->strstart++;
    s->lookahead--;
  }
}

/* The raw body of src[first, n) written by a matcher that has walked src[0, first) (first <= 32 768, first <= n).
 * NULL with *out_len = 0: Queue.Full (the CLI driver), or bad arguments. */
uint8_t *prm_deflate_raw(const uint8_t *src, size_t n, size_t first, int level, int queue_len, int driver, int dynamic, int matcher,
                         size_t *out_len) {
  *out_len = 0;
  init_tables();
  if (level < 0 || level > 9 || queue_len < 4 || (queue_len & (queue_len - 1)) || first > n || first > WSIZE) return NULL;
  queue_t q = {(int *)calloc((size_t)queue_len, sizeof(int)), 0, 0, (unsigned)queue_len};
  out_t o = {NULL, 0, 0};
  lz_t *s = lz_new(driver == DRV_HIGHER ? 4 : level, &q, src, n, matcher);
  prime_walk(s, (int)first);
  enc_t e;
  memset(&e, 0, sizeof e);
  e.blk.kind = KIND_FIXED;
  e.q = &q;
  e.o = &o;
  e.k = K_FIRST_ENTRY;
  block_t *b = (block_t *)calloc(1, sizeof *b);
  int first_flush = 1, full = 0;
  for (;;) {
    int r = lz_compress(s);
    int rc;
    if (r == LZ_FLUSH) {
      if (driver == DRV_ZL && !first_flush) rc = enc_encode(&e, V_FLUSH, NULL);
      else {
        first_flush = 0;
        make_block(driver, dynamic, 0, s, b);
        rc = enc_encode(&e, V_BLOCK, b);
      }
      while (rc == R_BLOCK && driver != DRV_CLI) {
        make_block(driver, dynamic, 0, s, b);
        rc = enc_encode(&e, V_BLOCK, b);
      }
    } else {
      if (driver == DRV_CLI) {
        if (q_available(&q) == 0) {
          full = 1;
          break;
        }
        q_push(&q, Q_EOB);
      } else if (matcher && !q_end_with_eob(&q)) q_push(&q, Q_EOB);
      make_block(driver, dynamic, 1, s, b);
      (void)enc_encode(&e, V_BLOCK, b);
      break;
    }
  }
  free(q.buf);
  free(s);
  free(b);
  if (full) {
    free(o.p);
    return NULL;
  }
  *out_len = o.n;
  if (!o.p) o.p = (uint8_t *)malloc(1);
  return o.p;
}

void prm_free(void *p) { free(p); }
