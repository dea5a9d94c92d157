"""The dynamic block of DESIGN 3.4, restated in Python from that text, and what the dynamic-mode tests share: pure Python, test
code only.

Restatement.  lengths(freq, limit) is the code-length rule (Huffman's tree with its stated tie-breaks as two explicit queues, the
repair on the counts, the hand-out); optimum(freq) is the unrestricted Huffman cost by heapq, which no tie-break changes;
plan(p) is the histogram of deflatecases.parse's tokens, the three sets of lengths, HLIT / HDIST / HCLEN and the run-length
operations; cdata(p) writes the block with deflatewriter.dynamic where it is strictly shorter than what the fixed mode writes and
deflatecases.cdata otherwise; member(p) puts header and trailer around it.  Nothing here looks at the code under test.

Corpus.  corpus() is deflatecases.corpus() and the payloads added here; reach(corpus) is what the restatement's own tokens and
headers say the corpus reaches, REACH what it has to reach (tests/test_deflate_dynamic_host.py asserts it).

HCLEN.  The header names the code-length code's lengths in the order 16, 17, 18, 0, 8, 7, 9, ...: HCLEN = 4 would mean that no
code length other than 0 occurs, that is a block without an end-of-block code, which is no block.  A member without a match
has the distance length 1 (place 18 of 19 in that order), and a distance code over two or more of 30 symbols holds a length of
4 or less (place 12 or later).  So no block has HCLEN below 12, and REACH asks for HCLEN = 19 and, instead of 4, for
HCLEN_LEAST = 14, which the payload "spread-distances" is made to reach."""
import functools
import heapq
import random
import struct
import zlib

import deflatecases as D
import deflatewriter as dw

LIT, DIST, CL = 286, 30, 19
HCLEN_LEAST = 14


def lengths(freq, limit):
    """the code lengths of `freq` under `limit`, as DESIGN 3.4 states the rule"""
    out = [0] * len(freq)
    leaves = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    if not leaves:
        return out
    if len(leaves) == 1:
        out[leaves[0][1]] = 1
        return out
    # Huffman's tree: the two smallest weights are joined; among equal weights a leaf before a node, leaves in their order,
    # nodes in the order they were made
    weight = [f for f, _s in leaves]
    parent = [None] * len(leaves)
    nodes = []                                # (weight, index into weight / parent), in the order made
    next_leaf, next_node = 0, 0

    def take():
        nonlocal next_leaf, next_node
        if next_node >= len(nodes) or (next_leaf < len(leaves) and weight[next_leaf] <= nodes[next_node][0]):
            next_leaf += 1
            return next_leaf - 1
        next_node += 1
        return nodes[next_node - 1][1]

    for _ in range(len(leaves) - 1):
        a = take()
        b = take()
        weight.append(weight[a] + weight[b])
        parent.append(None)
        parent[a] = parent[b] = len(weight) - 1
        nodes.append((weight[-1], len(weight) - 1))
    depth = [0] * len(weight)
    for k in range(len(weight) - 2, -1, -1):
        depth[k] = depth[parent[k]] + 1
    count = [0] * (limit + 1)
    for k in range(len(leaves)):
        count[min(depth[k], limit)] += 1
    over = sum(c << (limit - d) for d, c in enumerate(count) if d) - (1 << limit)
    assert over >= 0
    for _ in range(over):
        d = max(d for d in range(1, limit) if count[d])
        count[d] -= 1
        count[d + 1] += 2
        count[limit] -= 1
    assert sum(c << (limit - d) for d, c in enumerate(count) if d) == 1 << limit
    at = 0
    for d in range(limit, 0, -1):             # in the symbols' order, the longest first
        for _ in range(count[d]):
            out[leaves[at][1]] = d
            at += 1
    return out


def optimum(freq):
    """(sum of f * depth, depth) of an unrestricted Huffman code: the sum is the same for every tie-break; the depth is that of
    the tree that keeps itself as flat as the ties allow"""
    heap = [(f, 0) for f in freq if f > 0]
    if len(heap) < 2:
        return sum(f for f, _d in heap), len(heap)
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        total += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return total, heap[0][1]


def kraft_ok(lens, limit):
    """complete and within the limit, or the single code of one bit, or no code at all"""
    used = [l for l in lens if l]
    if len(used) <= 1:
        return used in ([], [1])
    return max(used) <= limit and sum(1 << (limit - l) for l in used) == 1 << limit


def cost(freq, lens):
    return sum(f * l for f, l in zip(freq, lens))


def tokens_of(chunks):
    return [t if isinstance(t, int) else t[:2] for tokens in chunks for t in tokens]


def histogram(chunks):
    lit, dist = [0] * LIT, [0] * DIST
    for t in tokens_of(chunks):
        if isinstance(t, int):
            lit[t] += 1
        else:
            lit[dw.length_symbol(t[0])] += 1
            dist[dw.distance_symbol(t[1])] += 1
    lit[dw.EOB] += 1
    return lit, dist


def plan(p, chunks=None):
    """everything the dynamic block of `p` is made of: a dict"""
    chunks = D.parse(p) if chunks is None else chunks
    lit_f, dist_f = histogram(chunks)
    lit, dist = lengths(lit_f, 15), lengths(dist_f, 15)
    hlit = max(257, max(s + 1 for s, l in enumerate(lit) if l))
    hdist = max([1] + [s + 1 for s, l in enumerate(dist) if l])
    if not any(dist):
        dist[0] = 1
    ops = dw.run_length_ops(lit[:hlit]) + dw.run_length_ops(dist[:hdist])
    cl_f = [0] * CL
    for s, _e in ops:
        cl_f[s] += 1
    cl = lengths(cl_f, 7)
    hclen = max(4, max(k + 1 for k, s in enumerate(dw.CL_ORDER) if cl[s]))
    header_bits = 17 + 3 * hclen + sum(cl[s] + (0 if s < 16 else (2, 3, 7)[s - 16]) for s, _e in ops)
    token_bits = 0
    for t in tokens_of(chunks):
        if isinstance(t, int):
            token_bits += lit[t]
        else:
            ls, ds = dw.length_symbol(t[0]), dw.distance_symbol(t[1])
            token_bits += lit[ls] + dw.LENGTH_EXTRA[ls - 257] + dist[ds] + dw.DIST_EXTRA[ds]
    bits = header_bits + token_bits + lit[dw.EOB]
    return {"chunks": chunks, "lit_freq": lit_f, "dist_freq": dist_f, "cl_freq": cl_f, "lit": lit, "dist": dist, "cl": cl, "hlit": hlit,
            "hdist": hdist, "hclen": hclen, "ops": ops, "header_bits": header_bits, "bytes": (bits + 7) // 8}


def today_bytes(p, chunks):
    """what the fixed mode writes for `p`: the fixed block, or the stored one"""
    f = D.fixed_bytes(chunks)
    return 5 + len(p) if len(p) > 0 and f >= 5 + len(p) else f


def cdata(p, chunks=None):
    chunks = D.parse(p) if chunks is None else chunks
    q = plan(p, chunks)
    if not q["bytes"] < today_bytes(p, chunks):
        return D.cdata(p, chunks)
    out = dw.write([dw.dynamic(tokens_of(chunks), q["lit"][:q["hlit"]], q["dist"][:q["hdist"]],
                               header={"ops": q["ops"], "cl_lengths": q["cl"], "hclen": q["hclen"], "hlit": q["hlit"], "hdist": q["hdist"]})])
    assert len(out) == q["bytes"]
    return out


def member(p, chunks=None):
    c = cdata(p, chunks)
    return D.HEADER + struct.pack("<H", len(c) + 25) + c + struct.pack("<II", zlib.crc32(p) & 0xFFFFFFFF, len(p))


# ---- histograms for the code-length rule -----------------------------------------------------------------------------------------
def fibonacci(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


@functools.lru_cache(maxsize=None)
def histograms():
    """((name, freq tuple, limit)): random ones, one and two used symbols, all equal, and Fibonacci ones whose tree is deeper
    than the limit over 286, over 30 and over 19 symbols"""
    r = random.Random(20240917)
    out = []
    for k in range(24):
        n, limit = ((LIT, 15), (DIST, 15), (CL, 7))[k % 3]
        top = (3, 40, 70000)[k // 3 % 3]
        zeros = r.random() * 0.8
        out.append(("random-%d" % k, tuple(0 if r.random() < zeros else r.randrange(1, top) for _ in range(n)), limit))
    for n, limit in ((LIT, 15), (DIST, 15), (CL, 7)):
        out.append(("none-%d" % n, (0,) * n, limit))
        out.append(("one-%d" % n, tuple(7 if s == n - 2 else 0 for s in range(n)), limit))
        out.append(("two-%d" % n, tuple((5, 1)[s % 2] if s in (3, n - 1) else 0 for s in range(n)), limit))
        out.append(("equal-%d" % n, (9,) * n, limit))
        out.append(("ones-%d" % n, (1,) * n, limit))
    fib = fibonacci(44)
    shuffled = list(fib)
    r.shuffle(shuffled)
    out.append(("fibonacci-286", tuple(shuffled[s // 6] if s % 6 == 0 and s // 6 < 44 else 0 for s in range(LIT)), 15))
    out.append(("fibonacci-286-dense", tuple(fib[s] if s < 40 else 1 + s % 3 for s in range(LIT)), 15))
    out.append(("fibonacci-30", tuple(fibonacci(30)), 15))
    out.append(("fibonacci-30-reversed", tuple(reversed(fibonacci(30))), 15))
    out.append(("fibonacci-19", tuple(fibonacci(19)), 7))
    out.append(("fibonacci-19-part", tuple(f if s % 2 else 0 for s, f in enumerate(fibonacci(19))), 7))
    out.append(("depth-16", tuple(fibonacci(17)) + (0,) * 13, 15))       # one level too deep ...
    out.append(("depth-15", tuple(fibonacci(16)) + (0,) * 14, 15))       # ... and the deepest that fits
    out.append(("depth-8", tuple(fibonacci(9)) + (0,) * 10, 7))
    out.append(("depth-7", tuple(fibonacci(8)) + (0,) * 11, 7))
    return tuple(out)


# ---- the corpus ------------------------------------------------------------------------------------------------------------------
def _edge(want):
    """the first payload of a fixed family whose dynamic block is `want` bytes above (0) or below (1) what is written today"""
    for seed in range(4000):
        r = random.Random(seed)
        n = r.randrange(40, 400)
        k = r.randrange(2, 40)
        p = bytes(r.randrange(k) * 5 for _ in range(n))
        chunks = D.parse(p)
        if today_bytes(p, chunks) - plan(p, chunks)["bytes"] == want:
            return p
    raise AssertionError("no payload found")


def _spread_distances(n, seed):
    """16 letters, and words of 8 copied from distances spread evenly over the distance symbols 5 .. 20: code lengths that keep
    away from 1, 2 and 13 .. 15 on both sides, which is what makes HCLEN small"""
    r = random.Random(seed)
    out = bytearray(r.randrange(16) for _ in range(2100))
    while len(out) < n:
        s = 5 + r.randrange(16)
        d = dw.DIST_BASE[s] + r.randrange(1 << dw.DIST_EXTRA[s])
        if r.random() < 0.5 and 8 <= d <= len(out):
            out += out[len(out) - d:len(out) - d + 8]
        out.append(r.randrange(16))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def added():
    r = random.Random(20240918)
    out = []
    out.append(("edge-equal", _edge(0)))                       # D = what is written today: today's bytes stay
    out.append(("edge-one-below", _edge(1)))                   # D one byte below: the dynamic block
    out.append(("two-literals-63", bytes(63)))                 # n < 64: empty lanes; literals only (HDIST = 1, one code of one bit)
    out.append(("literals-300", bytes(r.randrange(97, 101) for _ in range(300))))
    out.append(("one-distance", (b"abcdefg" * 400)[:64 * 40]))  # every match at distance 7: exactly one distance symbol
    out.append(("length-258", bytes(64 * 600)))                # length 258 used: HLIT = 286
    # a run of more than 138 zero lengths (no literal between 0x20 and 0xff but a few), repeats of a length beyond 6
    out.append(("sparse-letters", bytes(r.choice(b"\x01\x02\x03\xf0\xf1") for _ in range(2000))))
    out.append(("flat-64", bytes(r.randrange(64) for _ in range(8000))))           # 64 literals of nearly one length: 16s
    out.append(("all-bytes", bytes(range(256)) * 16 + bytes(r.randrange(256) for _ in range(4096))))
    out.append(("skewed", bytes(min(255, int(r.expovariate(0.05))) for _ in range(30000))))   # lengths 1 .. 15 in the header
    out.append(("spread-distances", _spread_distances(40000, 0)))
    for n in (3000, 20000):
        out.append(("text-%d" % n, D._text(n, n)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def corpus():
    return D.corpus() + added()


REACH = {
    "flags": {"dynamic", "fixed-kept", "stored-kept", "edge-one-below", "edge-equal", "literals-only", "one-distance-symbol",
              "many-distance-symbols", "hlit-257", "hlit-286", "op-16", "op-17", "op-18", "zero-run-above-138", "repeat-run-above-6",
              "hclen-19", "hclen-least", "header-ends-inside-lane-1s-byte", "empty-lanes", "n-0-fixed"},
}


def reach(cases):
    """what the restatement says `cases` reach, in the terms of REACH; also the least HCLEN of a block that is written"""
    got, least = set(), 19
    for _name, p in cases:
        n = len(p)
        chunks = D.parse(p)
        q = plan(p, chunks)
        today, f = today_bytes(p, chunks), D.fixed_bytes(chunks)
        if n == 0:
            assert q["bytes"] >= today
            got.add("n-0-fixed")
        if q["bytes"] == today:
            got.add("edge-equal")
        if q["bytes"] >= today:
            got.add("stored-kept" if n > 0 and f >= 5 + n else "fixed-kept")
            continue
        got.add("dynamic")
        if q["bytes"] == today - 1:
            got.add("edge-one-below")
        used_dist = sum(1 for f_ in q["dist_freq"] if f_)
        if used_dist == 0:
            assert q["hdist"] == 1 and q["dist"][:1] == [1]
            got.add("literals-only")
        if used_dist == 1:
            got.add("one-distance-symbol")
        if used_dist >= 8:
            got.add("many-distance-symbols")
        if q["hlit"] in (257, 286):
            got.add("hlit-%d" % q["hlit"])
        lens = q["lit"][:q["hlit"]] + q["dist"][:q["hdist"]]
        got |= {"op-%d" % s for s, _e in q["ops"] if s >= 16}
        for part in (q["lit"][:q["hlit"]], q["dist"][:q["hdist"]]):
            i = 0
            while i < len(part):
                run = 1
                while i + run < len(part) and part[i + run] == part[i]:
                    run += 1
                if part[i] == 0 and run > 138:
                    got.add("zero-run-above-138")
                if part[i] != 0 and run - 1 > 6:
                    got.add("repeat-run-above-6")
                i += run
        assert dw.expand_ops(q["ops"]) == lens
        least = min(least, q["hclen"])
        if q["hclen"] == 19:
            got.add("hclen-19")
        if q["hclen"] <= HCLEN_LEAST:
            got.add("hclen-least")
        if 0 < n < D.LANES:
            got.add("empty-lanes")
        lane1 = sum(q["lit"][t] if isinstance(t, int) else 1 for t in chunks[1])
        if q["header_bits"] % 8 and chunks[1] and lane1:
            lane0 = sum(q["lit"][t] for t in chunks[0] if isinstance(t, int))
            if (q["header_bits"] + lane0) % 8 and all(isinstance(t, int) for t in chunks[0]) and q["header_bits"] // 8 == (q["header_bits"] + lane0) // 8:
                got.add("header-ends-inside-lane-1s-byte")
    return got, least
