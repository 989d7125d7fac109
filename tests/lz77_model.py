"""A second witness for the lazy match finder: De.Lz77 (lib/de.ml:4013-4515, matcher 0, hash4) and Lz (lib/lz.ml,
matcher 1, the 3-byte rolled hash) restated in plain Python from the reference's text, in absolute positions.

Three entry points, each the model of one thing the GPU computes (tests/lz77_cases.py states its cases in their terms):

  links(data, matcher)             what deflate_link_kernel writes: per inserted position the distance to the latest
                                   earlier position with its hash, and the two tail heads of position len - 3
  look_ahead(data, matcher, level) what deflate_match_kernel computes: longest_match entered with prev_length = 2 at
                                   every position, over the full chain and over its first max_chain >> 2 candidates
  parse(data, matcher, level, q)   the whole matcher: the commands of every queue fill with the automatic EOBs, the
                                   two histograms, and a trace of every longest_match call and every emitted match

parse keeps the reference's own 64 KiB window (fill_window, slide_hash), so what is read beyond the end of the data is
what the reference reads there: zeros before the first slide, the bytes 32 KiB back after it.  The whole input arrives in
one piece followed by the end of input, as in oracle/de_deflate.c's drivers.

TEST INFRASTRUCTURE ONLY."""
from collections import namedtuple

MIN_MATCH, MAX_MATCH = 3, 258
MIN_LOOKAHEAD = MAX_MATCH + MIN_MATCH + 1
WBITS = 15
WSIZE = 1 << WBITS
MAX_DIST = WSIZE - MIN_LOOKAHEAD
TOO_FAR = 4096
HASH_BITS = 15
HASH_MASK = (1 << HASH_BITS) - 1
EOB = 256
COPY = 0x2000000

Cfg = namedtuple("Cfg", "good_length max_lazy nice_length max_chain")
# lib/de.ml:4031-4049; lib/lz.ml:143-148 has the same rows 4..9
LEVELS = {1: Cfg(4, 4, 8, 4), 2: Cfg(4, 5, 16, 8), 3: Cfg(4, 6, 32, 32), 4: Cfg(4, 4, 16, 16), 5: Cfg(8, 16, 32, 32),
          6: Cfg(8, 16, 128, 128), 7: Cfg(8, 32, 128, 256), 8: Cfg(32, 128, 258, 1024), 9: Cfg(32, 258, 258, 4096)}


def config(matcher, level):
    """the row a level runs at: Lz has no levels below 4 (lib/lz.ml:535)"""
    if matcher == 1 and level < 4:
        level = 4
    return LEVELS[level]


def hash4(b0, b1, b2, b3):
    v = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24)
    return ((v * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def hash3(b0, b1, b2):
    """update_hash rolled over three bytes from any state: shift 5, 15 bits"""
    h = 0
    for c in (b0, b1, b2):
        h = ((h << 5) ^ c) & HASH_MASK
    return h


def fp16(b0, b1, b2):
    """the fingerprint the link kernel keeps beside a link (deflate_common.hpp fp16)"""
    return (((b0 | (b1 << 8) | (b2 << 16)) * 0x9E3779B1) & 0xFFFFFFFF) >> 16


def p_end(data, matcher):
    """positions inserted whatever the matcher decides: those with 4 (De) / 3 (Lz) bytes of data"""
    n = len(data)
    if matcher == 1:
        return n - 2 if n >= 3 else 0
    return n - 3 if n >= 4 else 0


def pos_hash(data, matcher, p):
    return hash3(data[p], data[p + 1], data[p + 2]) if matcher else hash4(data[p], data[p + 1], data[p + 2], data[p + 3])


def heads(data, matcher):
    """per inserted position the latest earlier position with its hash, 0 = none (position 0 is NIL: the reference
    cannot tell it from an empty bucket), and the table after the last insertion"""
    table, prev = {}, []
    for p in range(p_end(data, matcher)):
        h = pos_hash(data, matcher, p)
        prev.append(table.get(h, 0))
        table[h] = p
    return prev, table


def links(data, matcher):
    """-> (dist[p] for the inserted positions, (tail0, tail1)).  dist is 0 where nothing lies within 32 767.  The tail
    heads are those of De's position len - 3, whose hash takes a 4th byte from beyond the data: 0, or the byte 32 KiB
    earlier (what the window holds there after a slide); absolute positions, 0 = none.  Lz: (0, 0)."""
    prev, table = heads(data, matcher)
    dist = [p - c if c and p - c <= 32767 else 0 for p, c in enumerate(prev)]
    n = len(data)
    tails = [0, 0]
    if matcher == 0 and n >= 4:
        for k in (0, 1):
            b3 = data[n - WSIZE] if k == 1 and n >= WSIZE else 0
            tails[k] = table.get(hash4(data[n - 3], data[n - 2], data[n - 1], b3), 0)
    elif matcher == 0 and n == 3:
        tails = [0, 0]
    return dist, tuple(tails)


def _lcp(buf, a, b, limit):
    if buf[a:a + limit] == buf[b:b + limit]:
        return limit
    n = 0
    while buf[a + n:a + n + 16] == buf[b + n:b + n + 16]:
        n += 16
    while n < limit and buf[a + n] == buf[b + n]:
        n += 1
    return n


Look = namedtuple("Look", "full quarter walked share3 near_end")


def look_ahead(data, matcher, level, positions=None):
    """per inserted position (or for the given ones only, as a dict) what longest_match returns when entered with prev_length = 2: (length, distance) over the
    full chain and over its first max_chain >> 2 candidates (length 2, distance 0: nothing), the number of candidates
    the full walk looks at, and whether one of them shares 3 bytes with the position.  The head is a candidate at
    distance <= MAX_DIST (lib/de.ml:4360), a later link only below it (cur_match > limit, :4140); the walk stops at the
    first candidate of nice_length; a later candidate wins only when it is longer.  Positions with less than
    MIN_LOOKAHEAD bytes in front of the end are marked: their lengths are clipped to the data here, the reference's
    depend on what its window holds beyond."""
    cfg = config(matcher, level)
    prev, _ = heads(data, matcher)
    n = len(data)
    q = cfg.max_chain >> 2
    out = [] if positions is None else {}
    for p in (range(len(prev)) if positions is None else positions):
        best, bdist = 2, 0
        quarter = None
        walked, share3 = 0, False
        room = min(MAX_MATCH, n - p)
        c = prev[p]
        if c and p - c <= MAX_DIST:
            while True:
                walked += 1
                share3 = share3 or data[c:c + 3] == data[p:p + 3]
                if best >= room or data[c + best] == data[p + best]:  # (only such a candidate can be longer)
                    ln = _lcp(data, c, p, room)
                    if ln > best:
                        best, bdist = ln, p - c
                if walked == q:
                    quarter = (best, bdist)
                if best >= cfg.nice_length or walked == cfg.max_chain:
                    break
                c = prev[c]
                if not c or p - c >= MAX_DIST:
                    break
        if quarter is None:
            quarter = (best, bdist)
        look = Look((best, bdist), quarter, walked, share3, p + MIN_LOOKAHEAD > n)
        if positions is None:
            out.append(look)
        else:
            out[p] = look
    return out


def _length_code(ln):
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    k = 0
    while k + 1 < len(base) and base[k + 1] <= ln:
        k += 1
    return k


def _dist_code(d):
    base = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
            6145, 8193, 12289, 16385, 24577]
    k = 0
    while k + 1 < len(base) and base[k + 1] <= d:
        k += 1
    return k


Call = namedtuple("Call", "pos bar budget walked length dist more")
Match = namedtuple("Match", "pos length dist deferrals")
Parse = namedtuple("Parse", "cmds lits dists calls matches slides")


def parse(data, matcher, level, queue=4096):
    """-> Parse(cmds, lits, dists, calls, matches, slides): the commands of every queue fill in order (for a tuple of
    queue sizes: a dict of such lists by size; literal = the
    byte, copy = COPY | (length - 3) << 16 | (distance - 1), EOB = 256: those the matcher pushes itself when one cell is
    left, lib/de.ml:4240-4243, and De's at the end of the input - Lz pushes none there), the literal/length and distance
    histograms, every longest_match call (position, bar = prev_length, budget, candidates looked at, result, and whether
    the budget ended the walk with a candidate in reach left), every
    emitted match with the number of deferrals in front of it, and the positions at which the window slid.

    Positions are absolute; `base` is the absolute position of window index 0.  Index 0 is NIL in the reference, and a
    slide drops what lies below the new base (slide_hash), so a head or a link <= base is NIL here."""
    data = bytes(data)
    n = len(data)
    good, max_lazy, nice, max_chain = config(matcher, level)
    w = bytearray(2 * WSIZE + 320)
    head = [0] * (1 << HASH_BITS)
    prev = {}
    base = ipos = ss = la = 0
    eoi = False
    rolled = 0  # Lz's hash state
    match_start = 0
    match_length = (MIN_MATCH - 1) if matcher else 0
    match_available = False
    queues = (queue,) if isinstance(queue, int) else tuple(queue)
    sinks = [[[], q, q, False] for q in queues]  # commands, capacity, free cells, "the last push filled it"
    lits, dists = [0] * 286, [0] * 30
    lits[256] = 1
    calls, matches, slides = [], [], []
    deferrals = 0

    def push(cmd):  # a push that leaves one free cell is followed by an EOB; the caller then empties the queue
        for sink in sinks:  # (the queue decides nothing else: several capacities can be filled in one pass)
            sink[0].append(cmd)
            sink[2] -= 1
            sink[3] = sink[2] == 1
            if sink[3]:
                sink[0].append(EOB)
                sink[2] = sink[1]

    while True:
        if la < MIN_LOOKAHEAD:
            # fill_window, lib/de.ml:4294-4342: slide when strstart has reached wsize + max_dist, then take what fits
            more = 2 * WSIZE - la - (ss - base)
            if ss - base >= WSIZE + MAX_DIST:
                keep = WSIZE - more
                w[0:keep] = w[WSIZE:WSIZE + keep]
                base += WSIZE
                slides.append(ss)
                more += WSIZE
            if eoi:
                if la == 0:
                    break
            elif ipos == n:
                eoi = True
                continue
            else:
                ln = min(more, n - ipos)
                o = ss + la - base
                w[o:o + ln] = data[ipos:ipos + ln]
                la += ln
                ipos += ln
                if matcher and la >= MIN_MATCH:  # lib/lz.ml:410-411: the rolled hash is primed again
                    rolled = ((w[ss - base] << 5) ^ w[ss - base + 1]) & HASH_MASK
                if la < MIN_LOOKAHEAD:
                    continue
        # deflate, one position: lib/de.ml:4351-4410
        s = ss - base
        hash_head = 0
        if la >= MIN_MATCH:
            if matcher:
                h = rolled = ((rolled << 5) ^ w[s + 2]) & HASH_MASK
            else:
                h = (((w[s] | (w[s + 1] << 8) | (w[s + 2] << 16) | (w[s + 3] << 24)) * 0x9E3779B1) & 0xFFFFFFFF) >> 17
            hash_head = head[h]
            if hash_head <= base:
                hash_head = 0
            prev[ss] = hash_head
            head[h] = ss
        prev_length, prev_match = match_length, match_start
        match_length = MIN_MATCH - 1
        if hash_head and prev_length < max_lazy and ss - hash_head <= MAX_DIST:
            # longest_match, lib/de.ml:4110-4174
            limit = ss - MAX_DIST if s > MAX_DIST else base
            budget = max_chain >> 2 if prev_length >= good else max_chain
            best, walked, cur, more = prev_length, 0, hash_head, False
            while True:
                walked += 1
                c = cur - base
                if w[c + best] == w[s + best] and w[c] == w[s]:  # only such a candidate can be longer
                    ln = 0
                    while ln < MAX_MATCH and w[c + ln] == w[s + ln]:
                        ln += 1
                    if ln > best:
                        match_start, best = cur, ln
                        if ln >= nice:
                            break
                cur = prev.get(cur, 0)
                if cur <= limit or walked == budget:
                    more = cur > limit  # the budget ended the walk with a candidate in reach left
                    break
            ml = min(best, la)
            calls.append(Call(ss, prev_length, budget, walked, ml, ss - match_start, more))
            if not (ml == MIN_MATCH and ss - match_start > TOO_FAR):
                match_length = ml
        if prev_length >= MIN_MATCH and match_length <= prev_length:
            off = ss - 1 - prev_match
            max_insert = ss + la - MIN_MATCH
            matches.append(Match(ss - 1, prev_length, off, deferrals))
            deferrals = 0
            lits[257 + _length_code(prev_length)] += 1
            dists[_dist_code(off)] += 1
            push(COPY | ((prev_length - 3) << 16) | (off - 1))
            la -= prev_length - 1
            for ss in range(ss + 1, ss + prev_length - 1):
                if ss <= max_insert:
                    s = ss - base
                    if matcher:
                        h = rolled = ((rolled << 5) ^ w[s + 2]) & HASH_MASK
                    else:
                        h = (((w[s] | (w[s + 1] << 8) | (w[s + 2] << 16) | (w[s + 3] << 24)) * 0x9E3779B1) & 0xFFFFFFFF) >> 17
                    hh = head[h]
                    prev[ss] = hh if hh > base else 0
                    head[h] = ss
            match_available = False
            match_length = MIN_MATCH - 1
            ss += 1
            continue
        if prev_length >= MIN_MATCH:
            deferrals += 1  # the match at the position before gives way to a longer one here
        if match_available:
            lits[w[s - 1]] += 1
            push(w[s - 1])
        match_available = True
        ss += 1
        la -= 1
    # trailing, lib/de.ml:4257-4266 / lib/lz.ml:348-354
    if match_available:
        lits[w[ss - base - 1]] += 1
        push(w[ss - base - 1])
    for sink in sinks:
        if not matcher and not (match_available and sink[3]):
            sink[0].append(EOB)
    cmds = sinks[0][0] if isinstance(queue, int) else {sink[1]: sink[0] for sink in sinks}
    return Parse(cmds, lits, dists, calls, matches, slides)
