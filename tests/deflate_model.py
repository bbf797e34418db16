"""The DEFLATE encoder of svim_amd/csrc/deflate_core.hpp stated a second time, from the rules in its comments and from RFC 1951 / RFC 1952 / BGZF, in plain
Python: lists, dicts and one big integer as the bit string.  No numpy, no zlib, no lanes, no staging window.  tests/test_deflate_encode_cases.py holds the host
build to it phase by phase, tests/test_gpu_deflate_encode_cases.py the kernels.

    match(text)            -> tokens, histogram            what def_match leaves
    codes(hist, n, crc)    -> dict (the DefBlockCodes content; codes_words() lays it out as the 692 words)
    bits(text, tokens, c)  -> the block's bytes
    parse(block)           -> the structure of a BGZF block, by a small inflate of its own

A token is a literal byte 0..255 or a pair (length, distance); token_words() gives the encoder's words."""

NL, ND, NHIST = 288, 32, 320
BLOCK, MAXPRE = 65280, 360
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# RFC 1951 section 3.2.5, written out: (first length, extra bits) of symbols 257..285 and (first distance, extra bits) of symbols 0..29
LEN_BASE, LEN_EXTRA, DIST_BASE, DIST_EXTRA = [], [], [], []
_b = 3
for _s in range(28):
    _e = 0 if _s < 8 else (_s - 4) // 4
    LEN_BASE.append(_b), LEN_EXTRA.append(_e)
    _b += 1 << _e
LEN_BASE.append(258), LEN_EXTRA.append(0)
_b = 1
for _s in range(30):
    _e = 0 if _s < 4 else _s // 2 - 1
    DIST_BASE.append(_b), DIST_EXTRA.append(_e)
    _b += 1 << _e
assert LEN_BASE[27] + 31 == 258 and DIST_BASE[29] + (1 << 13) - 1 == 32768


def len_symbol(length):
    """3..258 -> (symbol - 257, extra bits, extra value); 258 has a symbol of its own"""
    if length == 258:
        return 28, 0, 0
    s = max(k for k in range(28) if LEN_BASE[k] <= length)
    return s, LEN_EXTRA[s], length - LEN_BASE[s]


def dist_symbol(dist):
    s = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


def token_words(tokens):
    return [t if isinstance(t, int) else 0x80000000 | (t[1] - 1) << 9 | (t[0] - 3) for t in tokens]


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def histogram(tokens):
    hist = [0] * NHIST
    for t in tokens:
        if isinstance(t, int):
            hist[t] += 1
        else:
            hist[257 + len_symbol(t[0])[0]] += 1
            hist[NL + dist_symbol(t[1])[0]] += 1
    hist[256] += 1
    return hist


# ---- match ------------------------------------------------------------------------------------------------------------------------------------------------
def _hash(text, p):
    x = text[p] | text[p + 1] << 8 | text[p + 2] << 16 | text[p + 3] << 24
    return ((x * 2654435761) & 0xffffffff) >> 20


def _common(text, a, p, maxl):
    k = 0
    while k < maxl and text[a + k] == text[p + k]:
        k += 1
    return k


def match(text):
    """Positions are looked at in batches of 64.  A position that has four bytes left has two candidates: the most recent position of an EARLIER batch with
    the same 12-bit hash (if its four bytes are the same and it is at most 32 768 back), and the position at the distance of the last match taken before
    this batch began.  The longer wins, a tie goes to the last distance; below 4 bytes there is no match.  The parse takes the match at the first uncovered
    position that has one, else a literal."""
    n = len(text)
    table, tokens = {}, []
    cur = rep = 0
    for base in range(0, n, 64):
        end = min(base + 64, n)
        found = {}
        for p in range(max(base, cur), end):
            if p + 4 > n:
                continue
            maxl = min(258, n - p)
            length = dist = 0
            c = table.get(_hash(text, p))
            if c is not None and p - c <= 32768 and text[c:c + 4] == text[p:p + 4]:
                length, dist = _common(text, c, p, maxl), p - c
            if rep and rep <= p and rep != dist and text[p - rep:p - rep + 4] == text[p:p + 4]:
                l2 = _common(text, p - rep, p, maxl)
                if l2 >= length:
                    length, dist = l2, rep
            if length >= 4:
                found[p] = (length, dist)
        for p in range(base, end):
            if p + 4 <= n:
                table[_hash(text, p)] = p
        while cur < end:
            if cur in found:
                tokens.append(found[cur])
                rep = found[cur][1]
                cur += found[cur][0]
            else:
                tokens.append(text[cur])
                cur += 1
    return tokens, histogram(tokens)


# ---- codes ------------------------------------------------------------------------------------------------------------------------------------------------
def huffman_depths(freq):
    """freq: counts with at least two nonzero -> {symbol: depth} of the tree the two-queue merge builds: leaves ascending by (count, symbol), made nodes in the
    order they are made; each step joins the two smallest fronts, a leaf before a node of the same count"""
    leaves = sorted((f, s) for s, f in enumerate(freq) if f)
    nodes = []                                   # (count, left, right); a child is ('leaf', symbol) or ('node', index)
    li = ni = 0
    while (len(leaves) - li) + (len(nodes) - ni) > 1:
        picked, total = [], 0
        for _ in range(2):
            if li < len(leaves) and (ni >= len(nodes) or leaves[li][0] <= nodes[ni][0]):
                picked.append(("leaf", leaves[li][1]))
                total += leaves[li][0]
                li += 1
            else:
                picked.append(("node", ni))
                total += nodes[ni][0]
                ni += 1
        nodes.append((total, picked[0], picked[1]))
    depth = {}
    stack = [(("node", len(nodes) - 1), 0)]
    while stack:
        (kind, k), d = stack.pop()
        if kind == "leaf":
            depth[k] = d
        else:
            stack.append((nodes[k][1], d + 1))
            stack.append((nodes[k][2], d + 1))
    return depth


def build_lengths(hist, maxbits, info=None):
    """code lengths of at most maxbits.  An alphabet with fewer than two used symbols gets a second one (symbol 0, or symbol 1 when 0 is the used one) with count
    1.  Depths beyond maxbits are cut to maxbits; then, while the Kraft sum is too large, one code of maxbits is dropped and the longest shorter code is
    replaced by two codes one bit longer (miniz).  The shortest lengths go to the largest (count, symbol).  info (a dict) receives the unrestricted depth and
    the steps of the rule."""
    freq = list(hist)
    if sum(1 for f in freq if f) < 2 and not freq[0]:
        freq[0] = 1
    if sum(1 for f in freq if f) < 2:
        freq[1] = 1
    depth = huffman_depths(freq)
    count = [0] * (maxbits + 1)
    for d in depth.values():
        count[min(d, maxbits)] += 1
    steps = 0
    while sum(count[i] << (maxbits - i) for i in range(1, maxbits + 1)) != 1 << maxbits:
        count[maxbits] -= 1
        i = max(k for k in range(1, maxbits) if count[k])
        count[i] -= 1
        count[i + 1] += 2
        steps += 1
    if info is not None:
        info["depth"], info["steps"] = max(depth.values()), steps
    ranked = sorted(((f, s) for s, f in enumerate(freq) if f), reverse=True)
    lens = [0] * len(freq)
    at = 0
    for bits_ in range(1, maxbits + 1):
        for _ in range(count[bits_]):
            lens[ranked[at][1]] = bits_
            at += 1
    return lens


def canonical(lens):
    """RFC 1951 section 3.2.2 -> codes as numbers read from their most significant bit"""
    maxb = max(lens)
    bl_count = [0] * (maxb + 2)
    for v in lens:
        if v:
            bl_count[v] += 1
    next_code, code = [0] * (maxb + 2), 0
    for b in range(1, maxb + 1):
        code = (code + bl_count[b - 1]) << 1
        next_code[b] = code
    out = []
    for v in lens:
        out.append(next_code[v] if v else 0)
        if v:
            next_code[v] += 1
    return out


def _reversed(code, length):
    return int(format(code, "0%db" % length)[::-1], 2) if length else 0


def run_lengths(seq):
    """the joined code lengths -> [(symbol, extra value)]: a run of zeros is cut into 18s of 138 while 11 or more are left, then one 17 if 3 or more are left,
    then single zeros; a run of a nonzero value is the value once, then 16s of 6 while 3 or more are left (the last 16 takes 3..6), then single values"""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
        out += [(v, 0)] * run
    return out


def codes(hist, n, crc, info=None):
    """-> dict: code (320 words: bit-reversed code | length << 16), pre and suf (items (value, bits)), size, kind (0 end-of-file, 1 stored, 2 dynamic), and what
    led there: lit_len, dist_len, hlit, hdist, hclen, cl (run-length sequence), clen, dyn_bits"""
    head = [(0x8b1f, 16), (0x0408, 16), (0, 16), (0, 16), (0xff00, 16), (0x0006, 16), (0x4342, 16), (0x0002, 16)]
    if n == 0:
        pre = head + [(0x001b, 16), (0x0003, 16), (0, 16), (0, 16), (0, 16), (0, 16)]
        return dict(code=[0] * NHIST, pre=pre, suf=[], size=28, kind=0)
    info = {} if info is None else info
    il, idist, icl = {}, {}, {}
    lit_len = build_lengths(hist[:286], 15, il)
    dist_len = build_lengths(hist[NL:NL + 30], 15, idist)
    lit_code, dist_code = canonical(lit_len), canonical(dist_len)
    code = [0] * NHIST
    for s in range(286):
        code[s] = _reversed(lit_code[s], lit_len[s]) | lit_len[s] << 16
    for s in range(30):
        code[NL + s] = _reversed(dist_code[s], dist_len[s]) | dist_len[s] << 16
    hlit = max([257] + [s + 1 for s in range(286) if lit_len[s]])
    hdist = max([1] + [s + 1 for s in range(30) if dist_len[s]])
    cl = run_lengths(lit_len[:hlit] + dist_len[:hdist])
    chist = [0] * 19
    for s, _ in cl:
        chist[s] += 1
    clen = build_lengths(chist, 7, icl)
    ccode = canonical(clen)
    hclen = max([4] + [k + 1 for k in range(19) if clen[ORDER[k]]])
    nbits = 3 + 14 + 3 * hclen + sum(clen[s] + CL_EXTRA.get(s, 0) for s, _ in cl)
    for s in range(286):
        nbits += hist[s] * (lit_len[s] + (LEN_EXTRA[s - 257] if s > 256 else 0))
    for s in range(30):
        nbits += hist[NL + s] * (dist_len[s] + DIST_EXTRA[s])
    dyn = (nbits + 7) // 8
    stored = dyn >= n
    size = 18 + (n + 5 if stored else dyn) + 8
    pre = head + [(size - 1, 16)]
    suf = []
    if stored:
        pre += [(1, 8), (n, 16), (~n & 0xffff, 16)]
    else:
        pre += [(1 | 2 << 1, 3), ((hlit - 257) | (hdist - 1) << 5 | (hclen - 4) << 10, 14)]
        pre += [(clen[ORDER[k]], 3) for k in range(hclen)]
        for s, x in cl:
            pre.append((_reversed(ccode[s], clen[s]) | x << clen[s], clen[s] + CL_EXTRA.get(s, 0)))
        suf.append((code[256] & 0xffff, code[256] >> 16))
        if nbits % 8:
            suf.append((0, 8 - nbits % 8))
    suf += [(crc & 0xffff, 16), (crc >> 16, 16), (n & 0xffff, 16), (n >> 16, 16)]
    info.update(lit=il, dist=idist, cl=icl)
    return dict(code=code, pre=pre, suf=suf, size=size, kind=1 if stored else 2, lit_len=lit_len, dist_len=dist_len, hlit=hlit, hdist=hdist, hclen=hclen,
                cl=cl, clen=clen, dyn_bits=nbits, dyn=dyn)


def codes_words(c):
    """the 692 words of DefBlockCodes: code[320], pre[360], suf[8], n_pre, n_suf, size, kind; unused words 0"""
    item = lambda v, b: v | b << 24      # noqa: E731
    pre, suf = [item(*x) for x in c["pre"]], [item(*x) for x in c["suf"]]
    assert len(pre) <= MAXPRE and len(suf) <= 8
    return list(c["code"]) + pre + [0] * (MAXPRE - len(pre)) + suf + [0] * (8 - len(suf)) + [len(pre), len(suf), c["size"], c["kind"]]


# ---- bits -------------------------------------------------------------------------------------------------------------------------------------------------
def token_item(t, code):
    """(value, bits) of one token under the 320 code words: code, extra value, and for a match the distance code and its extra value, lowest bit first"""
    if isinstance(t, int):
        return code[t] & 0xffff, code[t] >> 16
    value = nb = 0
    ls, le, lx = len_symbol(t[0])
    ds, de, dx = dist_symbol(t[1])
    for v, b in ((code[257 + ls] & 0xffff, code[257 + ls] >> 16), (lx, le), (code[NL + ds] & 0xffff, code[NL + ds] >> 16), (dx, de)):
        value |= v << nb
        nb += b
    return value, nb


def items(text, tokens, c):
    out = list(c["pre"])
    if c["kind"] == 2:
        out += [token_item(t, c["code"]) for t in tokens]
    elif c["kind"] == 1:
        out += [(b, 8) for b in text]
    return out + list(c["suf"])


def bits(text, tokens, c):
    """every item appended to one integer, lowest bit first -> bytes (the last byte filled with zeros)"""
    acc = at = 0
    for v, b in items(text, tokens, c):
        acc |= (v & ((1 << b) - 1)) << at
        at += b
    return acc.to_bytes((at + 7) // 8, "little")


def block(text, crc):
    """one text of at most 65 280 bytes through the three phases -> its BGZF block"""
    tokens, hist = match(text) if text else ([], [0] * NHIST)
    c = codes(hist, len(text), crc)
    out = bits(text, tokens, c)
    assert len(out) == c["size"]
    return out


# ---- parse ------------------------------------------------------------------------------------------------------------------------------------------------
class _Bits(object):
    def __init__(self, data):
        self.v, self.at, self.n = int.from_bytes(data, "little"), 0, 8 * len(data)

    def take(self, k):
        assert self.at + k <= self.n, "the payload ends inside an item"
        x = (self.v >> self.at) & ((1 << k) - 1)
        self.at += k
        return x


def _decoder(lens):
    """{(length, code read from its first bit): symbol}, Kraft sum as a fraction of 2^15"""
    table = {(v, c): s for s, (v, c) in enumerate(zip(lens, canonical(lens))) if v}
    return table, sum(1 << (15 - v) for v in lens if v)


def _symbol(rd, table):
    code = 0
    for length in range(1, 16):
        code = code << 1 | rd.take(1)
        if (length, code) in table:
            return table[(length, code)], length
    raise AssertionError("no code of the table matches")


def parse(blk):
    """one BGZF block -> dict: kind, isize, crc, size and, for a dynamic block, hlit / hdist / hclen, clen (19 lengths), cl [(symbol, extra value)], lit_len /
    dist_len with kraft_lit / kraft_dist / kraft_cl (each must be exactly 2^15), tokens, widths (bits of every token item), eob_bits, pad (bits), text"""
    assert blk[:4] == b"\x1f\x8b\x08\x04" and blk[10:16] == b"\x06\x00BC\x02\x00", "BGZF header"
    size = (blk[16] | blk[17] << 8) + 1
    assert size == len(blk), "BSIZE"
    out = dict(size=size, crc=int.from_bytes(blk[-8:-4], "little"), isize=int.from_bytes(blk[-4:], "little"))
    payload = blk[18:-8]
    rd = _Bits(payload)
    assert rd.take(1) == 1, "one final block"
    btype = rd.take(2)
    if btype == 0:
        assert rd.take(5) == 0
        n, nn = rd.take(16), rd.take(16)
        assert n ^ nn == 0xffff and len(payload) == 5 + n
        out.update(kind="stored", text=bytes(payload[5:]))
    elif btype == 1:
        assert blk == EOF_BLOCK, "a fixed block is the end-of-file block only"
        out.update(kind="eof", text=b"")
    else:
        assert btype == 2
        hlit, hdist, hclen = rd.take(5) + 257, rd.take(5) + 1, rd.take(4) + 4
        assert hlit <= 286 and hdist <= 30
        clen = [0] * 19
        for k in range(hclen):
            clen[ORDER[k]] = rd.take(3)
        ctab, kraft_cl = _decoder(clen)
        assert kraft_cl == 1 << 15, "the code-length code is not complete"
        cl, seq = [], []
        while len(seq) < hlit + hdist:
            s, _ = _symbol(rd, ctab)
            x = rd.take(CL_EXTRA.get(s, 0))
            cl.append((s, x))
            if s < 16:
                seq.append(s)
            elif s == 16:
                assert seq, "16 with nothing before it"
                seq += [seq[-1]] * (3 + x)
            else:
                seq += [0] * ((3 if s == 17 else 11) + x)
        assert len(seq) == hlit + hdist, "a run crosses the end of the lengths"
        lit_len, dist_len = seq[:hlit] + [0] * (286 - hlit), seq[hlit:] + [0] * (30 - hdist)
        ltab, kraft_lit = _decoder(lit_len)
        dtab, kraft_dist = _decoder(dist_len)
        assert kraft_lit == 1 << 15 and kraft_dist == 1 << 15, "a code is not complete"
        tokens, widths, text = [], [], bytearray()
        while True:
            s, w = _symbol(rd, ltab)
            if s == 256:
                eob = w
                break
            if s < 256:
                tokens.append(s)
                text.append(s)
            else:
                assert s <= 285
                lx = rd.take(LEN_EXTRA[s - 257])
                ds, dw = _symbol(rd, dtab)
                assert ds < 30
                dx = rd.take(DIST_EXTRA[ds])
                length, dist = LEN_BASE[s - 257] + lx, DIST_BASE[ds] + dx
                assert dist <= len(text), "a distance reaches in front of the block"
                w += LEN_EXTRA[s - 257] + dw + DIST_EXTRA[ds]
                tokens.append((length, dist))
                for _ in range(length):
                    text.append(text[-dist])
            widths.append(w)
        pad = -rd.at % 8
        assert rd.take(pad) == 0 and rd.at == rd.n, "padding"
        out.update(kind="dynamic", hlit=hlit, hdist=hdist, hclen=hclen, clen=clen, cl=cl, lit_len=lit_len, dist_len=dist_len, kraft_lit=kraft_lit,
                   kraft_dist=kraft_dist, kraft_cl=kraft_cl, tokens=tokens, widths=widths, eob_bits=eob, pad=pad, text=bytes(text))
    assert out["isize"] == len(out["text"])
    return out
