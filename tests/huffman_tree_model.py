"""A second, slow implementation of De.T (lib/de.ml:1828-2191): the Huffman trees of a dynamic block and the run-length
pass over their lengths.  It is written from the algorithm's description, not from the oracle (oracle/de_deflate.c)
or the kernel (csrc/deflate_kernel.hip), so that an error those two share shows:

    t = make(freqs, length, max_length)     # t.lengths, t.codes, t.max_code, t.depth, t.limited
    plain_depth(freqs)                      # the depth of the tree without a limit
    scan(lit_lens, dist_lens)               # the 19 code-length frequencies of a header

The algorithm.  The used symbols (the two-symbol minimum: while fewer than two are used, symbol max_code + 1 while
max_code < 2, else symbol 0, joins with count 1) form a binary heap in symbol order, made a heap from the middle
down.  A key is (count, depth of the subtree); "a before b" holds when a's count is smaller, or the counts are equal
and a's depth is not larger - so of two equal keys the one asked about first wins, and which of two equal nodes leaves
first depends on where the heap holds them.  A sinking key goes to the right child when right is before left.  Each
step takes the first node out (the last slot takes its place and sinks), pairs it with the node then first, and puts
their parent (sum of the counts, larger depth + 1) into the first slot, where it sinks.  A leaf's length is its depth
below the root.  With a limit: every node deeper than the limit counts as one overflow and is put on the limit;
while overflow remains, one leaf of the longest length below the limit that has leaves moves one level down, takes
one leaf from the limit as its sibling, and the overflow drops by two; then the leaves, walked in the order they left
the heap (rarest first), receive the lengths from the limit upwards, as many of each as are counted.  Codes are the
canonical ones of RFC 1951 3.2.2 over symbols 0 .. max_code, bit-reversed.

The truth is lib/de.ml.  libz's trees.c, which De.T was ported from, agrees with it in every case tests/
test_huffman_trees.py compares (Z_HUFFMAN_ONLY blocks); where the two legitimately differ - libz picks the block kind
by its own costs and ends a block after 32 767 symbols - de.ml wins, and such outputs are not compared."""
from collections import namedtuple

Tree = namedtuple("Tree", "lengths codes max_code depth limited")
REP_3_6, REPZ_3_10, REPZ_11_138 = 16, 17, 18


def _before(a, b):
    """key a goes before key b: smaller count, or the same count and no deeper"""
    return a[0] < b[0] or (a[0] == b[0] and a[1] <= b[1])


def _sink(heap, key, slot):
    """the node in `slot` sinks to its place (heap[0] is not used)"""
    node, last = heap[slot], len(heap) - 1
    while 2 * slot <= last:
        child = 2 * slot
        if child < last and _before(key[heap[child + 1]], key[heap[child]]):
            child += 1
        if _before(key[node], key[heap[child]]):
            break
        heap[slot] = heap[child]
        slot = child
    heap[slot] = node


def _merge(freqs, length):
    """-> (parent of every node, the nodes in the order they left the heap, max_code, the root)"""
    used = [s for s in range(length) if freqs[s]]
    max_code = used[-1] if used else -1
    key = {s: (freqs[s], 0) for s in used}
    while len(used) < 2:
        if max_code < 2:
            max_code += 1
            extra = max_code
        else:
            extra = 0
        used.append(extra)
        key[extra] = (1, 0)
    heap = [None] + used
    for slot in range(len(used) // 2, 0, -1):
        _sink(heap, key, slot)
    parent, left_in_order, node = {}, [], length
    while len(heap) > 2:
        first = heap[1]
        heap[1] = heap[-1]
        heap.pop()
        _sink(heap, key, 1)
        second = heap[1]
        left_in_order += [first, second]
        key[node] = (key[first][0] + key[second][0], max(key[first][1], key[second][1]) + 1)
        parent[first] = parent[second] = node
        heap[1] = node
        node += 1
        _sink(heap, key, 1)
    return parent, left_in_order, max_code, heap[1]


def make(freqs, length, max_length=15):
    """the tree of freqs[0 .. length - 1]; `depth` is the longest code before the limit, `limited` whether any node was
    deeper than max_length (so the redistribution ran)"""
    parent, order, max_code, root = _merge(list(freqs) + [0] * max(0, length - len(freqs)), length)
    deep = {root: 0}
    for n in reversed(order):  # parents leave the heap after their children
        deep[n] = deep[parent[n]] + 1
    leaves = [n for n in order if n < length]
    depth = max(deep[n] for n in leaves)
    overflow = sum(1 for n in order if deep[n] > max_length)
    lens = [0] * length
    for n in leaves:
        lens[n] = min(deep[n], max_length)
    if overflow:
        count = [0] * (max_length + 1)
        for n in leaves:
            count[lens[n]] += 1
        while overflow > 0:
            b = max(l for l in range(1, max_length) if count[l])
            count[b] -= 1
            count[b + 1] += 2
            count[max_length] -= 1
            overflow -= 2
        todo = iter(leaves)
        for l in range(max_length, 0, -1):
            for _ in range(count[l]):
                lens[next(todo)] = l
    # canonical codes, most significant bit first, then reversed
    nxt, code = {}, 0
    for l in range(1, max(lens) + 1):
        code = (code + lens.count(l - 1) * (l > 1)) << 1
        nxt[l] = code
    codes = [0] * length
    for s in range(max_code + 1):
        if lens[s]:
            codes[s] = int(format(nxt[lens[s]], "0%db" % lens[s])[::-1], 2)
            nxt[lens[s]] += 1
    return Tree(lens, codes, max_code, depth, depth > max_length)


def plain_depth(freqs):
    """the longest code of the tree when nothing limits it"""
    return make(freqs, len(freqs), len(freqs) + 1).depth


def _runs(lens):
    out = []
    for l in lens:
        if out and out[-1][0] == l:
            out[-1][1] += 1
        else:
            out.append([l, 1])
    return out


def scan(lit_lens, dist_lens):
    """the frequencies of the 19 code-length symbols for a header that sends lit_lens (symbols 0 .. max_code of the
    literal/length tree) and then dist_lens (likewise), each list run-length coded on its own: a run of zeros goes in
    pieces of at most 138 (3-10: one 17, 11-138: one 18, shorter: single zeros); any other run of 4 and more sends its
    length once and then 16s that repeat it up to 6 times each, a last piece of 1 or 2 as single lengths; a run of
    up to 3 goes as single lengths"""
    bl = [0] * 19
    for lens in (lit_lens, dist_lens):
        for val, n in _runs(lens):
            if val == 0:
                while n:
                    k = min(n, 138)
                    n -= k
                    if k < 3:
                        bl[0] += k
                    else:
                        bl[REPZ_3_10 if k <= 10 else REPZ_11_138] += 1
                continue
            if n < 4:
                bl[val] += n
                continue
            bl[val] += 1  # the length itself, then up to 6 repeats of it
            bl[REP_3_6] += 1
            n -= 1 + min(n - 1, 6)
            while n:
                k = min(n, 6)
                n -= k
                if k < 3:
                    bl[val] += k
                else:
                    bl[REP_3_6] += 1
    return bl
