"""Raw DEFLATE streams (RFC 1951) built decision by decision, for the decoders of svim_amd/csrc/inflate_core.hpp and inflate_lanes.hpp.

Every other compressed stream of the suite comes out of zlib's compressor, which never writes a large part of what the format allows (distances above
32 506, a block longer than 16 383 symbols, empty blocks in mid-stream, length 258 as symbol 284 + 31, a dynamic header without a distance code ...).
htslib (libdeflate), htsjdk (igzip), zlib-ng and the Go / Rust encoders all write such streams.  Here the TEST takes every decision a compressor takes:

    Stream().stored(data) / .fixed(tokens) / .dynamic(tokens, ...)      block type and BFINAL per block
    tokens                  int = literal; (length, distance) = match; (258, distance, True) = length 258 as symbol 284 with extra bits 31;
                            ("L", symbol) / ("D", symbol, extra) = one raw literal/length / distance symbol (for streams that break a rule)
    dynamic(ll=, dl=)       code lengths of the two alphabets: a list, or a helper called with the symbol frequencies (huffman_lengths: length-limited
                            Huffman; skewed(m): longest code exactly m bits; flat_lengths: as flat as possible)
    dynamic(hlit=, hdist=, hclen=, cl_lens=, rle=, items=)   the header fields and how the code-length sequence is run-length coded

Written from RFC 1951 alone.  CORPUS is the named, deterministic set of streams the tests run: (name, group, deflate bytes, expected) with expected =
the payload, or INVALID for a stream zlib refuses (tests/test_deflate_streams.py holds every label to zlib's own verdict before a decoder of ours sees
the stream).  Standard library only; the "other encoders" payloads take their BAM-like records from svim_amd.synth when the corpus is built.

Test infrastructure only."""
import heapq
import random
import struct

INVALID = "INVALID"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
RING = 4096                 # bytes of recent output the wave decoder keeps in LDS (INF_RING)
FLUSH_AT = 1039             # pending bytes that make it flush (INF_FLUSH_AT)

LEN_BASE, LEN_EXTRA = [], []
for _i in range(29):
    _x = 0 if _i < 8 or _i == 28 else (_i - 4) >> 2
    LEN_EXTRA.append(_x)
    LEN_BASE.append(3 + _i if _i < 8 else (258 if _i == 28 else 3 + ((4 + (_i & 3)) << _x)))
DIST_BASE, DIST_EXTRA = [], []
for _i in range(30):
    _x = 0 if _i < 4 else (_i - 2) >> 1
    DIST_EXTRA.append(_x)
    DIST_BASE.append(1 + _i if _i < 4 else 1 + ((2 + (_i & 1)) << _x))
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32


def length_symbol(n):
    """(symbol - 257, extra value) of match length n, the way every encoder writes it (258 -> symbol 285)"""
    if n == 258:
        return 28, 0
    i = 28
    while LEN_BASE[i] > n or i == 28:
        i -= 1
    return i, n - LEN_BASE[i]


def dist_symbol(d):
    i = 29
    while DIST_BASE[i] > d:
        i -= 1
    return i, d - DIST_BASE[i]


class BitWriter(object):
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        """n bits, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 256:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def align(self):
        if self.n & 7:
            self.bits(0, 8 - (self.n & 7))

    def raw(self, data):
        assert self.n & 7 == 0
        self.buf += self.acc.to_bytes(self.n >> 3, "little") + bytes(data)
        self.acc = self.n = 0

    def bit_length(self):
        return 8 * len(self.buf) + self.n

    def getvalue(self):
        return bytes(self.buf) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def canonical_codes(lens):
    """code lengths -> [(bit-reversed code, length)] per symbol (RFC 1951 3.2.2); over-subscribed lengths still get codes (cut to their length)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if not l:
            out.append((0, 0))
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def kraft(lens, limit=15):
    """sum of 2^(limit - length): 2^limit for a complete code"""
    return sum(1 << (limit - l) for l in lens if l)


# ---- code-length helpers: each takes the symbol frequencies and returns one length per symbol (0 = unused) ------------------------------------------
def _spread(freqs, depth_counts):
    """lengths (counts per depth) handed to the used symbols, the shortest to the most frequent"""
    used = sorted((i for i, f in enumerate(freqs) if f), key=lambda i: (-freqs[i], i))
    ls = [d for d, c in enumerate(depth_counts) for _ in range(c)]
    assert len(ls) == len(used)
    out = [0] * len(freqs)
    for i, l in zip(used, ls):
        out[i] = l
    return out


def huffman_lengths(freqs, limit=15):
    """length-limited Huffman code: the Huffman tree, lengths above the limit cut to it and the Kraft sum repaired"""
    used = [i for i, f in enumerate(freqs) if f]
    out = [0] * len(freqs)
    if len(used) < 2:
        for i in used:
            out[i] = 1
        return out
    heap = [(freqs[i], i, None, None) for i in used]
    heapq.heapify(heap)
    tick = len(freqs)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tick, a, b))
        tick += 1
    stack = [(heap[0], 0)]
    while stack:
        (f, i, a, b), d = stack.pop()
        if a is None:
            out[i] = d
        else:
            stack += [(a, d + 1), (b, d + 1)]
    if max(out) > limit:
        for i in used:
            out[i] = min(out[i], limit)
        order = sorted(used, key=lambda i: (-out[i], freqs[i], i))        # longest and rarest first
        k = kraft(out, limit)
        while k > 1 << limit:
            i = next(i for i in order if out[i] < limit)
            k -= 1 << (limit - out[i] - 1)
            out[i] += 1
            order.sort(key=lambda i: (-out[i], freqs[i], i))
        for i in sorted(used, key=lambda i: (out[i], -freqs[i], i)):      # give back what the repair took too much of
            while out[i] > 1 and k + (1 << (limit - out[i])) <= 1 << limit:
                k += 1 << (limit - out[i])
                out[i] -= 1
    assert kraft(out, limit) == 1 << limit, "incomplete code from huffman_lengths"
    return out


def skewed(maxlen):
    """helper factory: a complete code whose longest code has exactly maxlen bits (needs maxlen + 1 <= used symbols <= 2^maxlen): one leaf per depth
    1 .. maxlen - 1, two at maxlen, the remaining symbols by splitting the deepest leaf above maxlen"""
    def fn(freqs):
        n = sum(1 for f in freqs if f)
        assert maxlen + 1 <= n <= 1 << maxlen, (n, maxlen)
        cnt = [0] + [1] * (maxlen - 1) + [2]
        for _ in range(n - maxlen - 1):
            d = max(d for d in range(1, maxlen) if cnt[d])
            cnt[d] -= 1
            cnt[d + 1] += 2
        out = _spread(freqs, cnt)
        assert max(out) == maxlen and kraft(out) == 1 << 15
        return out
    return fn


def flat_lengths(freqs):
    """as flat as possible: lengths k and k + 1 only"""
    n = sum(1 for f in freqs if f)
    if n < 2:
        return [1 if f else 0 for f in freqs]
    k = n.bit_length() - 1
    short = (2 << k) - n
    cnt = [0] * (k + 2)
    cnt[k], cnt[k + 1] = short, n - short
    return _spread(freqs, cnt)


def rle_items(seq, use16=True, use17=True, use18=True):
    """the code-length sequence as (symbol 0..18, extra value) items, greedily with the run symbols allowed"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and (use17 or use18):
            while run >= 11 and use18:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            while run >= 3 and use17:
                k = min(run, 10)
                out.append((17, k - 3))
                run -= k
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3 and use16:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
        i = j
    return out


def item_spans(items):
    """(start, end) in the code-length sequence of every item"""
    at, out = 0, []
    for s, x in items:
        k = 1 if s < 16 else (3 + x if s < 18 else 11 + x)
        out.append((at, at + k))
        at += k
    return out


# ---- the stream -------------------------------------------------------------------------------------------------------------------------------------
class Stream(object):
    """blocks appended one by one; .out is the payload the tokens stand for (raw symbols excepted)"""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.last_header = None          # of the last dynamic block: dict(items, hlit, hdist, hclen, ll, dl, cl)

    def _expand(self, tokens):
        out = self.out
        for t in tokens:
            if type(t) is int:
                out.append(t)
            elif t[0] not in ("L", "D"):
                n, d = t[0], t[1]
                assert 3 <= n <= 258 and 1 <= d <= 32768 and d <= len(out), t
                if d >= n:
                    out += out[len(out) - d:len(out) - d + n]
                else:
                    pat = bytes(out[len(out) - d:])
                    out += (pat * (n // d + 1))[:n]

    def _body(self, tokens, ll, dl, eob):
        lc, dc, w = canonical_codes(ll), canonical_codes(dl), self.w
        for t in tokens:
            if type(t) is int:
                c, n = lc[t]
                assert n, "literal %d has no code" % t
                w.bits(c, n)
            elif t[0] == "L":
                w.bits(*lc[t[1]])
            elif t[0] == "D":
                w.bits(*dc[t[1]])
                if t[1] < 30:
                    w.bits(t[2], DIST_EXTRA[t[1]])
            else:
                if len(t) > 2 and t[2]:
                    assert t[0] == 258
                    ls, lx = 27, 31
                else:
                    ls, lx = length_symbol(t[0])
                c, n = lc[257 + ls]
                assert n, "length symbol %d has no code" % (257 + ls)
                w.bits(c, n)
                w.bits(lx, LEN_EXTRA[ls])
                ds, dx = dist_symbol(t[1])
                c, n = dc[ds]
                assert n, "distance symbol %d has no code" % ds
                w.bits(c, n)
                w.bits(dx, DIST_EXTRA[ds])
        if eob:
            assert lc[256][1]
            w.bits(*lc[256])

    def stored(self, data, final=False, nlen=None):
        assert len(data) <= 65535
        self.w.bits(1 if final else 0, 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xffff) if nlen is None else nlen))
        self.w.raw(data)
        self.out += data
        return self

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        self._body(tokens, FIXED_LL, FIXED_DL, eob)
        self._expand(tokens)
        return self

    def reserved(self, final=True):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(3, 2)
        return self

    def dynamic(self, tokens, final=False, ll=huffman_lengths, dl=huffman_lengths, hlit=None, hdist=None, hclen=None, cl_lens=None, rle=(True, True, True),
                items=None, eob=True, pad_ll=(), pad_dl=()):
        """ll / dl: code lengths (list) or a helper called with the frequencies.  pad_ll / pad_dl: symbols counted as used although no token needs them.
        hlit / hdist: the COUNTS (257.., 1..) the header declares; default: up to the last used symbol.  cl_lens: the 19 lengths of the code-length code,
        or a helper; hclen: the count (4..19).  rle: (use16, use17, use18); items: the run-length coded sequence itself."""
        lf, df = [0] * 286, [0] * 30
        lf[256] = 1
        for s in pad_ll:
            lf[s] += 1
        for s in pad_dl:
            df[s] += 1
        for t in tokens:
            if type(t) is int:
                lf[t] += 1
            elif t[0] == "L":
                if t[1] < 286:
                    lf[t[1]] += 1
            elif t[0] == "D":
                if t[1] < 30:
                    df[t[1]] += 1
            else:
                lf[257 + (27 if len(t) > 2 and t[2] else length_symbol(t[0])[0])] += 1
                df[dist_symbol(t[1])[0]] += 1
        if callable(ll):
            if sum(1 for f in lf if f) < 2:
                lf[0 if lf[0] == 0 else 1] += 1       # (a second code, so that the set is complete)
            ll = ll(lf)
        if callable(dl):
            if sum(1 for f in df if f) == 1:
                df[0 if df[0] == 0 else 1] += 1
            dl = dl(df) if any(df) else [0]
        ll, dl = list(ll), list(dl)
        if hlit is None:
            hlit = max(257, max(i for i, l in enumerate(ll) if l) + 1) if any(ll) else 257
        if hdist is None:
            hdist = max(1, max([i for i, l in enumerate(dl) if l] + [0]) + 1)
        ll = (ll + [0] * 320)[:hlit]
        dl = (dl + [0] * 64)[:hdist]
        if items is None:
            items = rle_items(ll + dl, *rle)
        cf = [0] * 19
        for s, _ in items:
            cf[s] += 1
        if callable(cl_lens) or cl_lens is None:
            if sum(1 for f in cf if f) < 2:
                cf[0 if cf[0] == 0 else 1] += 1
            cl_lens = (cl_lens or (lambda f: huffman_lengths(f, 7)))(cf)
        if hclen is None:
            hclen = max(4, max(k for k, s in enumerate(CL_ORDER) if cl_lens[s]) + 1)
        w = self.w
        w.bits(1 if final else 0, 1)
        w.bits(2, 2)
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for k in range(hclen):
            w.bits(cl_lens[CL_ORDER[k]], 3)
        cc = canonical_codes(cl_lens)
        for s, x in items:
            w.bits(*cc[s])
            if s >= 16:
                w.bits(x, (2, 3, 7)[s - 16])
        self.last_header = dict(items=items, hlit=hlit, hdist=hdist, hclen=hclen, ll=ll, dl=dl, cl=list(cl_lens))
        self._body(tokens, (ll + [0] * 288)[:288], (dl + [0] * 32)[:32], eob)
        self._expand(tokens)
        return self

    def finish(self):
        return self.w.getvalue(), bytes(self.out)


# ---- payloads and parsers ---------------------------------------------------------------------------------------------------------------------------
def rand_bytes(seed, n, alphabet=None):
    rng = random.Random(seed)
    if alphabet is None:
        return rng.randbytes(n)
    return bytes(rng.choices(alphabet, k=n))


def greedy_tokens(data, window=32768, start=0, history=0):
    """greedy LZ77 parse of data[start:] (matches may reach into data[start - history:start]): the longest of the most recent candidates of a 3-byte
    hash, taken as soon as it is found"""
    table, out, i, n = {}, [], start, len(data)
    for j in range(max(0, start - history), start):
        table.setdefault(data[j:j + 3], []).append(j)
    while i < n:
        key = data[i:i + 3]
        best, bd = 0, 0
        cands = table.get(key)
        if cands and len(key) == 3:
            for c in reversed(cands[-6:]):
                if i - c > window:
                    break
                m, lim = 3, min(258, n - i)
                while m < lim and data[c + m] == data[i + m]:
                    m += 1
                if m > best:
                    best, bd = m, i - c
        if best >= 3:
            out.append((best, bd))
            for j in range(i, i + best):
                table.setdefault(data[j:j + 3], []).append(j)
            i += best
        else:
            out.append(data[i])
            table.setdefault(key, []).append(i)
            i += 1
    return out


def profile_payloads():
    """what the 'other encoders' policies compress: BAM-like record bytes, base qualities, FASTA text, 2-bit-skewed noise"""
    rng = random.Random(77)
    qual = bytes(min(60, max(2, int(rng.gauss(22, 9)))) for _ in range(30000))
    seq = "".join(rng.choices("ACGT", k=9000))
    fasta = (">chr1 test\n" + "\n".join((seq * 3)[i:i + 60] for i in range(0, 24000, 60)) + "\n").encode("ascii")
    noise = bytes(rng.choices((0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88, 0x00, 0xff),
                              weights=[12] * 16 + [1, 1], k=24000))
    import foreign_bam as FB
    from svim_amd import synth
    refs = synth.make_reference(3, [("chr1", 60000)])
    recs = synth.coordinate_sort(synth.planted_reads(5, 40, refs, ["chr1"], [60000], n_sites=6, types=("DEL", "INS")))
    bam = b"".join(FB.record_bytes(a, FB.decorate(rng, a, k), qual=[rng.randrange(2, 50) for _ in range(len(a._seq or ""))]) for k, a in enumerate(recs))[:40000]
    return [("bam", bam), ("qual", qual), ("fasta", fasta), ("noise2bit", noise)]


# ---- encoder policies (also what tests/foreign_bam.py takes as deflate=): payload -> raw DEFLATE ---------------------------------------------------
def policy_one_block(payload, tokens=None):
    """one dynamic block over the whole payload, greedy parse over a 32 KiB window (the shape of libdeflate's output; a stand-in, not its output)"""
    return Stream().dynamic(tokens if tokens is not None else greedy_tokens(payload), final=True).finish()[0]


def policy_short_blocks(payload, tokens=None, per_block=300):
    """many short dynamic blocks, each with its own tables"""
    tokens = tokens if tokens is not None else greedy_tokens(payload)
    s = Stream()
    if not tokens:
        return s.dynamic([], final=True).finish()[0]
    for i in range(0, len(tokens), per_block):
        s.dynamic(tokens[i:i + per_block], final=i + per_block >= len(tokens))
    return s.finish()[0]


def policy_static(payload, tokens=None):
    """fixed Huffman tables only"""
    return Stream().fixed(tokens if tokens is not None else greedy_tokens(payload), final=True).finish()[0]


POLICIES = {"one_block": policy_one_block, "short_blocks": policy_short_blocks, "static": policy_static}


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------------------
def _valid_cases(add):
    R = rand_bytes
    r32k = list(R(1, 32768))

    # -- distances
    toks, out_len = list(R(2, 300)), 300
    for ds in range(30):
        for x in (0, (1 << DIST_EXTRA[ds]) - 1):
            d = DIST_BASE[ds] + x
            if d > out_len:
                toks += list(R(100 + ds, d - out_len))
                out_len = d
            toks.append((5, d))
            out_len += 5
    add("dist/every-symbol-min-max-extra.fixed", "distances", Stream().fixed(toks, True))
    add("dist/every-symbol-min-max-extra.dynamic", "distances", Stream().dynamic(toks, True))
    toks = list(R(3, 40))
    for d in (1, 2, 3, 4, 15, 16, 17):
        toks += [(7, d), 65, (20, d), 66]
    add("dist/small-1-2-3-4-15-16-17", "distances", Stream().fixed(toks, True))
    for d in (4095, 4096, 4097, 32506, 32507, 32767, 32768):
        for alt in (False, True):
            s = Stream().fixed(r32k + [(258, d, alt), (3, d), (258, 1), (64, 2), (258, d, alt), (130, d)], True)
            add("dist/%d-%s" % (d, "sym284x31" if alt else "sym285"), "distances", s)
    add("dist/32768-source-at-offset-0", "distances", Stream().dynamic(r32k + [(258, 32768), 7, (3, 32768 - 0)], True, dl=skewed(9), pad_dl=range(20)))
    # ring size +- the pending bytes around a flush: literals up to k bytes before / after the flush threshold, then a match at 4096 -+ what is pending
    for pend in (FLUSH_AT - 17, FLUSH_AT - 1, FLUSH_AT, FLUSH_AT + 1, FLUSH_AT + 15, 2 * FLUSH_AT):
        toks = list(R(4, 8192 + pend))
        for d in (RING - pend, RING + pend, RING - 1, RING, RING + 1, RING - 1024, RING - 1024 - 258, RING - 1024 - 257):
            toks += [(258, d), (3, d), 9]
        add("dist/ring-around-flush-pending-%d" % pend, "distances", Stream().dynamic(toks, True))
    toks, pos = [], 0
    for step in (1, 2, 3, 17, 64, 65, 1000, 1039, 1040, 3071, 3072, 4095, 4096, 4097, 8191, 32768):
        step = min(step, 32768 - pos)                              # (the last one: distance 32 768)
        toks += list(R(5 + step, step))
        pos += step
        toks.append((min(258, max(3, pos)), pos))                 # distance = bytes produced so far: the first byte of the output
        pos += min(258, max(3, pos))
    add("dist/equal-to-bytes-produced", "distances", Stream().dynamic(toks, True))
    add("dist/equal-to-bytes-produced.fixed", "distances", Stream().fixed(toks, True))
    toks = list(R(6, 9000))
    for back in (RING - 1024 + 100, RING - 1024 + 1, RING - 1024, RING - 100, RING, RING + 100, RING + 257):
        toks += [(258, back), 1, 2, (200, back)]                 # the source starts beyond what the ring serves and ends inside it
    add("dist/source-from-global-memory-into-the-ring", "distances", Stream().dynamic(toks, True))

    # ... the same over a literal alphabet of 12 symbols: code tables small enough for a lane of the lane-per-block decoder (it gives up the tables of random bytes)
    A = b"ACGTNacgtn\n>"
    toks, out_len = list(R(2, 300, A)), 300
    for ds in range(30):
        for x in (0, (1 << DIST_EXTRA[ds]) - 1):
            d = DIST_BASE[ds] + x
            if d > out_len:
                toks += list(R(100 + ds, d - out_len, A))
                out_len = d
            toks.append((5, d))
            out_len += 5
    add("dist/every-symbol-min-max-extra.small-alphabet", "distances", Stream().dynamic(toks, True))
    a32k = list(R(1, 32768, A))
    for d in (1, 2, 3, 4, 15, 16, 17, 4095, 4096, 4097, 32506, 32507, 32767, 32768):
        s = Stream().dynamic(a32k + [(258, d, True), (3, d), (258, 1), (64, 2), (258, d), (130, d), 65, (4, d), (5, 3), (258, 3, True)], True)
        add("dist/%d.small-alphabet" % d, "distances", s)

    # -- lengths
    toks = list(R(7, 600))
    for ls in range(29):
        for x in sorted({0, (1 << LEN_EXTRA[ls]) - 1}):
            toks += [(LEN_BASE[ls] + x, 1 + 19 * ls), 200 + ls]
    toks += [(258, 300, True), (258, 1, True)]
    add("len/every-symbol-min-max-extra.fixed", "lengths", Stream().fixed(toks, True))
    add("len/every-symbol-min-max-extra.dynamic", "lengths", Stream().dynamic(toks, True))
    add("len/every-symbol-min-max-extra.small-alphabet", "lengths", Stream().dynamic(list(R(7, 600, A)) + [t for t in toks[600:] if type(t) is not int], True))
    add("len/258-as-285-and-as-284x31", "lengths", Stream().dynamic(list(R(8, 500)) + [(258, 400), (258, 400, True), 5, (258, 3, True), (258, 3)], True))
    # ... where the token is decoded by the serial path: symbol 284 on a 15-bit code, the distance on a 9-bit one (codes beyond the one-lookup tables)
    rare284 = lambda f: skewed(15)([(1 if i == 284 else 1000 + i) if x else 0 for i, x in enumerate(f)])
    s = Stream().dynamic(list(R(8, 700)) + [(258, 600, True), 5, (258, 3, True), (258, 699, True), (258, 1)], True, ll=rare284, dl=skewed(9), pad_dl=range(12))
    assert s.last_header["ll"][284] == 15
    add("len/258-as-284x31-on-long-codes", "lengths", s)
    toks = list(R(9, 10))
    for d in (1, 2, 3, 5):
        for n in (3, 4, 63, 64, 65, 258):
            toks += [d * 16 + 1, d + n & 255, (n, d)]
    add("len/overlapping-copies.fixed", "lengths", Stream().fixed(toks, True))
    add("len/overlapping-copies.dynamic", "lengths", Stream().dynamic(toks, True))
    add("len/overlapping-copies.small-alphabet", "lengths", Stream().dynamic([t if type(t) is not int else A[t % 12] for t in toks], True))
    for d in (1, 7, 258, 300):
        toks = list(R(10 + d, max(d, 10)))
        n = len(toks)
        while n + 258 <= 65536:
            toks.append((258, d))
            n += 258
        if 65536 - n >= 3:
            toks.append((65536 - n, d))
        else:
            toks += [0] * (65536 - n)
        s = Stream().dynamic(toks, True)
        assert len(s.out) == 65536
        add("len/chain-of-258-to-65536-dist-%d" % d, "lengths", s)
    add("len/match-ends-at-the-last-byte", "lengths", Stream().fixed(list(R(11, 5000)) + [(258, 4999)], True))
    add("len/match-ends-at-the-last-byte.65536", "lengths", Stream().dynamic(list(R(12, 65536 - 258)) + [(258, 33)], True))
    toks, pos = list(R(13, 800)), 800
    while (pos // 1024 + 1) * 1024 + 158 <= 65536:
        nxt = (pos // 1024 + 1) * 1024
        fill = nxt - pos - 100
        toks += list(R(pos, fill)) + [(258, 1 + pos % 900)]       # from 100 bytes before the multiple of 1024 to 158 behind it
        pos += fill + 258
    add("len/match-across-every-multiple-of-1024", "lengths", Stream().dynamic(toks, True))
    add("len/match-across-every-multiple-of-1024.fixed", "lengths", Stream().fixed(toks, True))

    # -- block structure
    for size in (65280, 65536):
        data = R(14, 3000, b"ACGTN\n") * 22
        data = data[:size]
        toks = greedy_tokens(data)
        s = Stream().dynamic(toks, True)
        assert len(s.out) == size and len(toks) > 200
        add("block/one-dynamic-block-%d" % size, "block structure", s)
        rng, toks, n = random.Random(size), [], 0
        while n < size - 20:                                                    # ~25 000 symbols in ONE block: literals with short and far matches between them
            if n > 100 and rng.random() < 0.3:
                t = (rng.randrange(3, 13), rng.randrange(1, min(n, 32768) + 1))
                n += t[0]
            else:
                t, n = rng.randrange(40, 90), n + 1
            toks.append(t)
        toks += [33] * (size - n)
        add("block/one-dynamic-block-%d-mixed-tokens" % size, "block structure", Stream().dynamic(toks, True))
        toks = list(R(15, size, bytes(range(40, 90))))
        add("block/one-dynamic-block-%d-literals" % size, "block structure", Stream().dynamic(toks, True))
    rng = random.Random(16)
    s = Stream()
    for k in range(200):
        kind = rng.randrange(3) if k else 0
        body = list(rng.randbytes(rng.randrange(0, 40)))
        if len(s.out) > 50 and kind:
            body += [(rng.randrange(3, 40), rng.randrange(1, min(len(s.out), 30000)))]
        if kind == 0:
            s.stored(bytes(rng.randbytes(rng.randrange(0, 60)) if k else rng.randbytes(64)), k == 199)
        elif kind == 1:
            s.fixed(body, k == 199)
        else:
            s.dynamic(body, k == 199)
    add("block/200-tiny-blocks-of-mixed-types", "block structure", s)
    s = Stream().stored(b"").stored(b"").fixed(list(R(17, 100))).stored(b"").dynamic(list(R(18, 100)) + [(50, 150)]).stored(b"").stored(b"").fixed([1, 2, 3, (3, 3)], True)
    add("block/empty-stored-blocks-start-between-before-final", "block structure", s)
    add("block/empty-stored-block-as-the-final-block", "block structure", Stream().fixed(list(R(19, 100))).stored(b"", True))
    phases = set()
    for k in range(8):                                                          # a fixed block of k 9-bit literals ends at bit (2 + k) % 8 of its byte
        s = Stream().fixed([200] * k)
        b = s.w.bit_length() & 7
        phases.add(b)
        s.stored(R(40 + k, 300)).dynamic([1, 2, 3, (30, 250)] + [77] * k)
        b2 = s.w.bit_length() & 7
        s.stored(R(30 + k, 33)).fixed([(100, 300), (258, 1)], True)
        add("block/stored-after-block-ends-at-bits-%d-and-%d" % (b, b2), "block structure", s)
    assert phases == set(range(8))
    add("block/stored-65535", "block structure", Stream().stored(R(41, 65535), True))
    add("block/stored-65000-then-matches-into-it", "block structure", Stream().stored(R(42, 65000)).fixed([(258, 32768), (258, 30000), (20, 3)], True))
    add("block/final-empty-fixed-block", "block structure", Stream().dynamic(list(R(43, 2000)) + [(100, 1500)]).fixed([], True))
    add("block/final-empty-dynamic-block", "block structure", Stream().fixed(list(R(44, 2000)) + [(100, 1500)]).dynamic([], True))
    add("block/final-empty-dynamic-block-after-stored", "block structure", Stream().stored(R(45, 5000)).dynamic([], True))
    s = Stream().stored(R(46, 3000)).fixed(list(R(47, 2000)) + [(258, 4000), (10, 5000)]).dynamic(list(R(48, 2500)) + [(258, 7000), (100, 2600), (50, 7800)])
    s.stored(R(49, 10)).fixed([(258, 8000), (200, 9), (258, 4200)]).dynamic([(258, 8600), (258, 300), (3, 9000)], True)
    add("block/matches-back-into-stored-fixed-dynamic-predecessors", "block structure", s)
    for k in (1, 2, 5, 14, 15):                                                # fewer bytes than lie in front of the destination's first 16-byte boundary: nothing to flush yet
        add("block/stored-%d-bytes-alone" % k, "block structure", Stream().stored(R(50 + k, k), True))
    add("block/stored-3-bytes-then-fixed", "block structure", Stream().stored(R(66, 3)).fixed([7, 8, 9, (3, 6)], True))
    add("block/output-0-bytes.stored", "block structure", Stream().stored(b"", True))
    add("block/output-0-bytes.fixed", "block structure", Stream().fixed([], True))
    add("block/output-0-bytes.dynamic", "block structure", Stream().dynamic([], True))

    # -- code tables
    lit = list(R(50, 6000, bytes(range(256))))                      # every literal occurs
    body = lit + [(3 + k, 1 + 7 * k) for k in range(200)] + lit[:500]
    for m in (9, 10, 11, 15):
        add("table/litlen-max-length-%d" % m, "code tables", Stream().dynamic(body, True, ll=skewed(m)))
    far = list(R(51, 33000))
    dbody = far + [x for ds in range(30) for x in ((4, DIST_BASE[ds]), ds)] * 3
    for m in (8, 9, 15):
        add("table/dist-max-length-%d" % m, "code tables", Stream().dynamic(dbody, True, dl=skewed(m)))
    add("table/litlen-15-and-dist-15", "code tables", Stream().dynamic(dbody + body, True, ll=skewed(15), dl=skewed(15)))
    add("table/code-length-code-max-length-7", "code tables", Stream().dynamic(body, True, ll=skewed(15), cl_lens=skewed(7)))
    allsym = list(range(256)) * 2 + far + [x for ls in range(29) for x in ((LEN_BASE[ls], 1 + ls), ls)] + [(3, DIST_BASE[ds]) for ds in range(30)]
    s = Stream().dynamic(allsym, True, ll=flat_lengths, dl=flat_lengths)
    assert all(s.last_header["ll"]) and s.last_header["hlit"] == 286 and all(s.last_header["dl"]) and s.last_header["hdist"] == 30
    add("table/complete-code-all-286-and-all-30-symbols", "code tables", s)
    s = Stream().dynamic(list(R(52, 4000)), True, hlit=257, dl=[0], hdist=1)
    add("table/hlit-257-literals-only+hdist-1-with-length-0", "code tables", s)
    s = Stream().dynamic(list(R(53, 900, b"ACGT")) + [0], True, dl=[0], hdist=1)
    add("table/hdist-1-with-length-0-no-distance-code", "code tables", s)
    s = Stream().dynamic(list(R(53, 900, b"ACGT")) + [0], True, dl=[0] * 30, hdist=30)
    add("table/hdist-30-all-lengths-0", "code tables", s)
    s = Stream().dynamic(list(R(54, 50)) + [(10, 1), 3, (258, 1), (3, 1)] * 20, True, dl=[1], hdist=1)
    add("table/single-distance-code-of-1-bit-used-by-matches", "code tables", s)
    s = Stream().dynamic(list(R(54, 50)) + [(10, 4), 3, (258, 4), (3, 4)] * 20, True, dl=[0, 0, 0, 1], hdist=4)
    add("table/single-distance-code-of-1-bit-symbol-3", "code tables", s)
    # the shortest header a valid block can have: HCLEN = 5 (16 17 18 0 8).  HCLEN = 4 leaves no non-zero code length at all - see the invalid group
    s = Stream().dynamic(list(R(55, 3000, bytes(range(1, 256)))), True, ll=[0] + [8] * 256, hlit=257, dl=[0], hdist=1, cl_lens=[2] + [0] * 7 + [1] + [0] * 7 + [0, 0, 2], rle=(False, False, True))
    assert s.last_header["hclen"] == 5 and max(s.last_header["cl"]) == 2
    add("table/hclen-5-smallest-valid+code-length-code-of-lengths-1-2", "code tables", s)
    sparse = [65] * 300 + [250] * 200 + [(3, 1), (20, 400)] * 30
    s = Stream().dynamic(sparse, True, rle=(False, False, True))
    assert {x for x, _ in s.last_header["items"]} & {16, 17, 18} == {18}
    add("table/code-lengths-with-18-runs-only", "code tables", s)
    s = Stream().dynamic(sparse, True, rle=(True, False, False))
    assert {x for x, _ in s.last_header["items"]} & {16, 17, 18} == {16}
    add("table/code-lengths-with-16-runs-only", "code tables", s)
    s = Stream().dynamic(body, True, ll=flat_lengths, rle=(False, False, False))
    add("table/code-lengths-without-runs", "code tables", s)
    # a run over the literal/length -> distance boundary: the last length lengths and the first distance lengths are equal
    ll = [0] * 286
    for i in (65, 66, 67, 68, 256, 257, 258, 259):
        ll[i] = 3
    s = Stream().dynamic([65, 66, 67, 68, (3, 1), (4, 2), (5, 3), 65], True, ll=ll, hlit=260, dl=[3, 3, 3, 3, 0, 0, 3, 3, 3, 3], hdist=10)
    sp = [b for b in item_spans(s.last_header["items"]) if b[0] < 260 < b[1]]
    assert sp and s.last_header["items"][item_spans(s.last_header["items"]).index(sp[0])][0] == 16
    add("table/16-run-across-the-literal-distance-boundary", "code tables", s)
    s = Stream().dynamic([65, 66] * 40 + [(3, 50), (3, 70), 65], True, ll=[0] * 65 + [2, 2] + [0] * 189 + [2, 2], hlit=270, dl=[0] * 11 + [1, 1], hdist=13)
    sp = [k for k, b in enumerate(item_spans(s.last_header["items"])) if b[0] < 270 < b[1]]
    assert sp and s.last_header["items"][sp[0]][0] == 18
    add("table/18-run-across-the-literal-distance-boundary", "code tables", s)
    # 15 bits right before 1 bit: the most frequent literal has the 1-bit code, the rarest ones 15 bits
    skew = [0] * 2000 + list(range(1, 40)) + [x for k in range(1, 11) for x in (k, 0)] * 4 + [(3, 1), 9, 0, (200, 60), 8, 0]
    s = Stream().dynamic(skew, True, ll=lambda f: skewed(15)([(10 ** 9 if i == 0 else (1 if i <= 10 else 1000 + i)) if x else 0 for i, x in enumerate(f)]))
    assert s.last_header["ll"][0] == 1 and set(s.last_header["ll"][1:11]) == {15}
    add("table/15-bit-code-then-1-bit-code", "code tables", s)
    eob_long = lambda f: skewed(15)([(1 if i == 256 else 1000 * x + i) if x else 0 for i, x in enumerate(f)])
    s = Stream().dynamic(list(R(56, 3000, bytes(range(30)))) + [(5, 7)], True, ll=eob_long)
    assert s.last_header["ll"][256] == 15
    add("table/end-of-block-is-the-longest-code", "code tables", s)
    s = Stream().dynamic(list(R(57, 200)) + [(5, 7)], ll=eob_long).fixed([(20, 100)]).dynamic(list(R(58, 80)), True, ll=eob_long)
    add("table/end-of-block-longest-then-more-blocks", "code tables", s)

    # -- input geometry
    rare = list(range(40, 256))                                     # 216 symbols on 15-bit codes, 20 frequent ones that are never used after the header
    freq = lambda f: skewed(15)([(1 if 40 <= i < 256 else 10 ** 6 + i) if x else 0 for i, x in enumerate(f)])
    s = Stream().dynamic(list(R(58, 30000, bytes(rare))) + [(30, 1000), (258, 29000)], True, ll=freq, pad_ll=range(0, 40))
    assert min(s.last_header["ll"][40:256]) >= 14
    add("input/body-of-15-bit-codes", "input geometry", s)
    for nsym, name in ((2, "1-bit"), (3, "1-2-bit"), (5, "2-3-bit")):
        toks = list(R(59, 20000, bytes(range(65, 65 + nsym - 1))))
        toks += [x for k in range(600) for x in ([65] * (10 + k % 50) + [(3 + k % 6, 1 + k % 9)])]
        s = Stream().dynamic(toks, True, dl=flat_lengths)
        add("input/body-of-%s-literals" % name, "input geometry", s)
    # multi-window steps (2, 3, 4 windows of 64 bits per step) are taken when a step yields at most half a byte per input bit: literals of 6-7 bits with short
    # matches at far distances between them, the shape of base qualities
    rng, toks, n = random.Random(62), list(R(62, 3000, bytes(range(33, 83)))), 3000
    while n < 40000:
        if rng.random() < 0.35:
            t = (rng.randrange(3, 6), rng.randrange(1, min(n, 32768) + 1) if rng.random() < 0.7 else rng.randrange(1, 40))
            n += t[0]
        else:
            t, n = rng.randrange(33, 83), n + 1
        toks.append(t)
    add("input/multi-window-steps-literals-and-short-matches", "input geometry", Stream().dynamic(toks, True, ll=flat_lengths))
    add("input/multi-window-steps-literals-and-short-matches.fixed", "input geometry", Stream().fixed(toks, True))
    toks = [x for k in range(2500) for x in ([65] * (k % 13) + [66] * (k % 5) + [(3 + k % 4, 2 + k % 11), 65 + k % 3])]
    add("input/short-matches-between-short-literals", "input geometry", Stream().dynamic([65, 66, 67] * 8 + toks, True))
    for target in (255, 256, 257, 511, 512, 513, 959, 960, 961, 962, 963, 964, 965, 1023, 1024, 1025, 1919, 1920, 1921, 1922, 1923, 1924, 2047, 2048, 2049):
        # fixed block of 8-bit literals: 3 + 8 n + 7 bits; the tail of 9-bit literals trims the stream to the byte
        n = target - 2
        s = Stream().fixed(list(R(60, n, bytes(range(100)))) + [(3, 5)], True)
        while len(s.finish()[0]) != target:
            n += target - len(s.finish()[0])
            s = Stream().fixed(list(R(60, n, bytes(range(100)))) + [(3, 5)], True)
        add("input/stream-of-%d-bytes" % target, "input geometry", s)
    for target in (1023, 1024, 1025):
        n = target * 8 // 15
        s = Stream().dynamic(list(R(61, n, bytes(rare))), True, ll=freq, pad_ll=range(0, 40))
        add("input/15-bit-body-stream-near-%d-bytes(%d)" % (target, len(s.finish()[0])), "input geometry", s)

    # -- "other encoders": stand-ins by construction (three fixed policies over seeded payloads), NOT output of libdeflate / igzip / zlib-ng
    for pname, payload in profile_payloads():
        toks = greedy_tokens(payload)
        for polname, pol in sorted(POLICIES.items()):
            add("profile/%s.%s" % (pname, polname), "other encoders", (pol(payload, toks), payload))


def _invalid_cases(add):
    R = rand_bytes
    base = list(R(70, 300))
    add("invalid/btype-3", "invalid: block type", Stream().reserved())
    add("invalid/btype-3-after-a-block", "invalid: block type", Stream().fixed(base).reserved())
    add("invalid/stored-len-nlen-mismatch", "invalid: stored", Stream().stored(R(71, 100), True, nlen=0xff9a))
    add("invalid/stored-len-nlen-equal", "invalid: stored", Stream().stored(R(71, 100), True, nlen=100))
    for hlit in (287, 288):
        add("invalid/hlit-%d" % hlit, "invalid: header counts", Stream().dynamic(base, True, ll=[8] * 256 + [9] * (hlit - 256 - 2) + [9, 9], hlit=hlit, dl=[1, 1]))
    for hdist in (31, 32):
        add("invalid/hdist-%d" % hdist, "invalid: header counts", Stream().dynamic(base, True, dl=[5] * hdist, hdist=hdist))
    add("invalid/code-length-code-over-subscribed", "invalid: code-length code", Stream().dynamic(base, True, cl_lens=[1, 1, 1] + [0] * 13 + [2, 2, 2], rle=(False, False, False)))
    add("invalid/code-length-code-incomplete", "invalid: code-length code", Stream().dynamic(base, True, cl_lens=lambda f: [l + 1 if l else 0 for l in huffman_lengths(f, 6)]))
    add("invalid/hclen-4-no-non-zero-length", "invalid: code-length code", Stream().dynamic([], True, ll=[0] * 257, hlit=257, dl=[0], hdist=1, cl_lens=[2] + [0] * 15 + [3, 3, 1],
                                                                                      items=[(18, 127), (18, 109)], eob=False))
    ll = huffman_lengths([1] * 257 + [0] * 29)
    add("invalid/repeat-16-as-the-first-entry", "invalid: code lengths", Stream().dynamic([], True, ll=ll, dl=[1, 1], items=[(16, 0)] + rle_items(ll[3:] + [1, 1]), eob=False))
    add("invalid/run-overshoots-hlit+hdist", "invalid: code lengths", Stream().dynamic([], True, ll=ll, dl=[1, 1], items=rle_items(ll + [1]) + [(16, 3)], eob=False))
    add("invalid/zero-run-overshoots-hlit+hdist", "invalid: code lengths", Stream().dynamic([], True, ll=ll, dl=[1, 0], items=rle_items(ll + [1]) + [(18, 5)], eob=False))
    noeob = huffman_lengths([1] * 256 + [0] * 30)
    add("invalid/no-end-of-block-code", "invalid: code lengths", Stream().dynamic(base, True, ll=noeob, dl=[1, 1], eob=False))
    add("invalid/litlen-over-subscribed", "invalid: literal/length set", Stream().dynamic(base, True, ll=[8] * 257 + [9] * 3, dl=[1, 1]))
    add("invalid/litlen-incomplete", "invalid: literal/length set", Stream().dynamic(base, True, ll=[9] * 257 + [0] * 29, dl=[1, 1]))
    add("invalid/litlen-incomplete-by-one-code", "invalid: literal/length set", Stream().dynamic(list(R(70, 300, bytes(range(200)))), True, ll=[8] * 254 + [0, 0, 8] + [0] * 29, dl=[1, 1]))
    add("invalid/litlen-single-code-of-2-bits", "invalid: literal/length set", Stream().dynamic([], True, ll=[0] * 256 + [2], dl=[0]))
    # ... with tables small enough for a lane of the lane-per-block decoder, and bodies that only use codes that exist
    few = [65] * 40 + [66] * 9
    add("invalid/litlen-incomplete.small-tables", "invalid: literal/length set", Stream().dynamic(few, True, ll=[0] * 65 + [1, 3] + [0] * 189 + [2], dl=[0]))
    add("invalid/litlen-over-subscribed.small-tables", "invalid: literal/length set", Stream().dynamic(few, True, ll=[0] * 65 + [1, 2] + [0] * 189 + [2, 2], dl=[0]))
    add("invalid/dist-incomplete-two-codes.small-tables", "invalid: distance set", Stream().dynamic(few + [(3, 1), (3, 2)], True, dl=[2, 2]))
    add("invalid/dist-incomplete-one-code-missing.small-tables", "invalid: distance set", Stream().dynamic(few + [(3, 1), (3, 2)], True, dl=[1, 2]))
    add("invalid/dist-single-code-of-2-bits.small-tables", "invalid: distance set", Stream().dynamic(few + [(3, 1)], True, dl=[2]))
    add("invalid/dist-over-subscribed.small-tables", "invalid: distance set", Stream().dynamic(few + [(3, 1)], True, dl=[1, 1, 1]))
    add("invalid/dist-over-subscribed", "invalid: distance set", Stream().dynamic(base + [(3, 1)], True, dl=[1, 1, 1]))
    add("invalid/dist-incomplete-two-codes", "invalid: distance set", Stream().dynamic(base + [(3, 1), (3, 2)], True, dl=[2, 2]))
    add("invalid/dist-incomplete-many-codes", "invalid: distance set", Stream().dynamic(base + [(3, 1), (3, 20)], True, dl=[5] * 30))
    add("invalid/dist-single-code-of-2-bits", "invalid: distance set", Stream().dynamic(base + [(3, 1)], True, dl=[2]))
    for sym in (286, 287):
        add("invalid/fixed-symbol-%d" % sym, "invalid: symbols", Stream().fixed(base + [("L", sym), ("D", 0, 0)], True))
    for sym in (30, 31):
        add("invalid/fixed-distance-symbol-%d" % sym, "invalid: symbols", Stream().fixed(base + [("L", 257), ("D", sym, 0)], True))
        add("invalid/fixed-distance-symbol-%d-after-literals-only" % sym, "invalid: symbols", Stream().fixed([65, ("L", 260), ("D", sym, 0)], True))
    add("invalid/distance-beyond-start-at-position-0", "invalid: distance too far", Stream().fixed([("L", 257), ("D", 0, 0)], True))
    add("invalid/distance-beyond-start-at-position-0.dynamic", "invalid: distance too far", Stream().dynamic([("L", 257), ("D", 0, 0)], True))
    for n, dsym, x in ((300, 16, 44), (5000, 24, 904), (32767, 29, 8191)):       # one byte beyond the start: distance n + 1
        assert DIST_BASE[dsym] + x == n + 1
        add("invalid/distance-one-beyond-start-at-%d" % n, "invalid: distance too far", Stream().fixed(list(R(72, n)) + [("L", 260), ("D", dsym, x), 1, 2, 3], True))
    add("invalid/distance-one-beyond-start-at-300.dynamic", "invalid: distance too far", Stream().dynamic(list(R(72, 300)) + [("L", 260), ("D", 16, 44)], True))
    add("invalid/distance-one-beyond-start-among-matches", "invalid: distance too far", Stream().fixed(list(R(72, 64)) + [(3, 5), (4, 9), ("L", 257), ("D", 12, 7), (3, 1)], True))
    add("invalid/distance-used-without-a-distance-code", "invalid: no distance code", Stream().dynamic(base + [("L", 257), ("D", 0, 0)], True, dl=[0], hdist=1))
    add("invalid/distance-used-without-a-distance-code-first-token", "invalid: no distance code", Stream().dynamic([("L", 257), ("D", 0, 0)] + base, True, dl=[0], hdist=1))
    add("invalid/unused-code-of-single-distance-code", "invalid: no distance code", _second_code_of_single(base))
    # streams that end early (the whole stream is sound, cut at a chosen byte)
    s15 = Stream().dynamic(list(R(73, 400, bytes(range(40, 256)))), True, ll=lambda f: skewed(15)([(1 if 40 <= i < 256 else 10 ** 6 + i) if x else 0 for i, x in enumerate(f)]),
                           pad_ll=range(0, 40)).finish()[0]
    add("invalid/ends-inside-a-code", "invalid: truncated", (s15[:len(s15) - 2], INVALID))
    add("invalid/ends-inside-a-code.last-byte", "invalid: truncated", (s15[:len(s15) - 1], INVALID))
    at_extra = Stream().fixed(list(R(74, 30000)) + [(9, 24577 + 3000)], True).finish()[0]
    add("invalid/ends-inside-extra-bits", "invalid: truncated", (at_extra[:len(at_extra) - 2], INVALID))
    st = Stream().fixed(base).stored(R(75, 1000), True).finish()[0]
    add("invalid/ends-inside-a-stored-run", "invalid: truncated", (st[:len(st) - 1], INVALID))
    add("invalid/ends-inside-a-stored-run.half", "invalid: truncated", (st[:len(st) - 500], INVALID))
    add("invalid/ends-inside-a-stored-header", "invalid: truncated", (st[:len(st) - 1002], INVALID))
    add("invalid/ends-before-the-final-block", "invalid: truncated", Stream().fixed(base).dynamic(base, False))
    add("invalid/ends-inside-a-dynamic-header", "invalid: truncated", (Stream().dynamic(base, True).finish()[0][:20], INVALID))
    for name, s in (("fixed", Stream().fixed(base + [(50, 100)], True)), ("dynamic", Stream().dynamic(base + [(50, 100)], True)), ("stored", Stream().stored(R(76, 350), True)),
                    ("dynamic-literal-last", Stream().dynamic(base + [(50, 100), 7], True))):
        d, out = s.finish()
        add("invalid/declared-size-one-too-small.%s" % name, "invalid: declared size", (d, INVALID, len(out) - 1))
        add("invalid/declared-size-one-too-large.%s" % name, "invalid: declared size", (d, INVALID, len(out) + 1))


def _second_code_of_single(base):
    """a single 1-bit distance code (symbol 0 = code 0): the stream uses the OTHER 1-bit code, which stands for nothing"""
    s = Stream().dynamic(base + [("L", 257)], True, dl=[1], hdist=1, eob=False)
    s.w.bits(1, 1)
    s.w.bits(*canonical_codes(s.last_header["ll"] + [0] * 40)[256])
    return s


def build_corpus():
    """[(name, group, deflate bytes, expected payload or INVALID, declared size)]: declared size = what the caller tells the decoder the stream inflates to
    (the ISIZE field of a BGZF block); for an invalid stream the size its sound twin would have, or an arbitrary one"""
    out, seen = [], set()

    def add(name, group, s):
        if isinstance(s, Stream):
            data, payload = s.finish()
            expected, size = (INVALID if group.startswith("invalid") else payload), len(payload)
        elif len(s) == 3:
            data, expected, size = s
        else:
            data, expected = s
            size = 1000 if expected == INVALID else len(expected)
        assert name not in seen, name
        seen.add(name)
        assert expected == INVALID or len(expected) <= 65536
        out.append((name, group, bytes(data), expected, size))
    _valid_cases(add)
    _invalid_cases(add)
    return out


_CORPUS = None


def corpus():
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = build_corpus()
    return _CORPUS


def write_corpus_file(path, entries):
    """the file the host tools read (--corpus): per entry u32 name length, name, u32 stream length, stream, u32 declared size, u8 valid"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(entries)))
        for name, _, data, expected, size in entries:
            nb = name.encode("ascii")
            fh.write(struct.pack("<I", len(nb)) + nb + struct.pack("<I", len(data)) + data + struct.pack("<IB", size, 0 if expected == INVALID else 1))
