"""Directed inputs for the phases of the DEFLATE encoder (svim_amd/csrc/deflate_core.hpp), shared by tests/test_deflate_encode_cases.py (host build) and
tests/test_gpu_deflate_encode_cases.py (kernels).  Everything is built by code from fixed seeds; what the encoder has to answer comes from
tests/deflate_model.py.  Every family states the edge it is there for and ASSERTS here, on the CPU, that its inputs reach it: a family that stops
reaching its edge fails when the cases are built.

    codes_cases()   [dict(name, hist, n, crc)]                      phase 2 alone: histograms no text of the suite gives
    bits_cases()    [dict(name, text, tokens, codes)]               phase 3 alone: token lists and (partly synthetic) DefBlockCodes
    match_texts()   [(name, text)]                                  phase 1, and all three phases: texts of at most one block
    COVERAGE        what the families reached (figures for DESIGN section 33)
"""
import functools
import random
import zlib

import deflate_model as M
import text_gz_cases as TC

COVERAGE = {}
K15 = 1 << 15


def runs(seq):
    out, i = [], 0
    while i < len(seq):
        k = 1
        while i + k < len(seq) and seq[i + k] == seq[i]:
            k += 1
        out.append((seq[i], k))
        i += k
    return out


# ---- histograms that give chosen code lengths -----------------------------------------------------------------------------------------------------------
def fill_kraft(lens, slots):
    """complete the set: the mass still missing from 1, in binary, as one code per set bit, put into `slots` in turn (two codes of one bit if nothing is used)"""
    rest = K15 - sum(K15 >> v for v in lens if v)
    assert rest >= 0
    todo = [1, 1] if rest == K15 else [v for v in range(1, 16) if rest & (K15 >> v)]
    assert len(todo) <= len(slots)
    for v, s in zip(todo, slots):
        assert lens[s] == 0
        lens[s] = v
    assert sum(K15 >> v for v in lens if v) == K15
    return lens


def dyadic_hist(lit_len, dist_len):
    """counts 2^(longest - length): the one histogram family whose Huffman lengths are forced (the code meets the entropy, so every optimal code has these
    lengths whatever the ties do)"""
    hist = [0] * M.NHIST
    for base, lens in ((0, lit_len), (M.NL, dist_len)):
        if any(lens):
            top = max(lens)
            for s, v in enumerate(lens):
                hist[base + s] = 1 << (top - v) if v else 0
    return hist


def _segments(segs, size):
    out = []
    for v, k in segs:
        out += [v] * k
    assert len(out) <= size
    return out + [0] * (size - len(out))


def _codes_case(name, hist, n=M.BLOCK, crc=None, **expect):
    return dict(name=name, hist=list(hist), n=n, crc=zlib.crc32(name.encode()) if crc is None else crc, expect=expect)


def _fib(k):
    out = [1, 1]
    while len(out) < k:
        out.append(out[-1] + out[-2])
    return out[:k]


# ---- limit15 --------------------------------------------------------------------------------------------------------------------------------------------
def _limit15():
    """unrestricted depth 15 (the limit not needed), 16, 17, 20 and the deepest the token budget of a block allows, on three alphabets; ties at the bottom"""
    rng = random.Random(1501)
    cases, deepest = [], 0
    lit_syms = list(range(256))
    for where in ("literals", "literals_lengths", "distances"):
        for want in (15, 16, 17, 20, "deepest"):
            found = None
            for attempt in range(4000):
                k = (want if want != "deepest" else 21) + 1 - rng.randrange(0, 3)
                counts = _fib(k) + [rng.choice(_fib(k)[:6]) for _ in range(rng.randrange(0, 5))]          # a chain, and a few more of the small counts: ties
                if want == "deepest":
                    counts = _fib(22) + [rng.choice([1, 1, 2, 3]) for _ in range(attempt % 4)]
                budget = M.BLOCK + (0 if where == "distances" else 1)
                if sum(counts) > budget:
                    continue
                depth = max(M.huffman_depths(counts).values())
                if depth == want or (want == "deepest" and depth >= 21):
                    found = counts
                    break
            assert found, (where, want)
            rng.shuffle(found)
            hist = [0] * M.NHIST
            if where == "distances":
                for s, f in zip(sorted(rng.sample(range(30), len(found))), sorted(found, reverse=True)):       # (few extra bits for the heavy ones: the block stays dynamic)
                    hist[M.NL + s] = f
                hist[65], hist[256] = 1000, 1
            else:
                pool = lit_syms + (list(range(257, 286)) if where == "literals_lengths" else [])
                syms = rng.sample(pool, len(found) - 1) + [256]                                              # the end-of-block symbol is one of the leaves
                for s, f in zip(syms, found):
                    hist[s] = f
                if hist[256] != 1:                                                                          # ... with its count of 1 (the chain has two of them)
                    other = [s for s in syms if hist[s] == 1][0]
                    hist[other], hist[256] = hist[256], 1
            info = {}
            c = M.codes(hist, M.BLOCK, 0, info)
            side = info["dist"] if where == "distances" else info["lit"]
            lens = c["dist_len"] if where == "distances" else c["lit_len"]
            assert max(lens) == 15 and c["kind"] == 2, (where, want)
            if want == 15:
                assert side["depth"] == 15 and side["steps"] == 0
            else:
                assert side["depth"] > 15 and side["steps"] >= 1 and (want == "deepest" or side["depth"] == want), (where, want, side)
            deepest = max(deepest, side["depth"])
            cases.append(_codes_case("limit15_%s_%s" % (where, want), hist, depth=side["depth"], steps=side["steps"]))
    # many steps: 200 leaves of count 1 (a subtree of depth 8) at the bottom of a chain; a leaf may weigh less than the node in front as long as the next leaf
    # weighs more than the node before (then the node is still the second of the two smallest)
    hist = [0] * M.NHIST
    for s in range(199):
        hist[s] = 1
    hist[256] = 1
    before, node, s = 200, 401, 200
    hist[199] = 201
    while node + before + 1 <= M.BLOCK + 1:
        hist[s] = before + 1
        before, node, s = node, node + before + 1, s + 1
    info = {}
    M.codes(hist, M.BLOCK, 0, info)
    assert info["lit"]["depth"] > 15 and info["lit"]["steps"] >= 50, info["lit"]
    cases.append(_codes_case("limit15_many_steps", hist, depth=info["lit"]["depth"], steps=info["lit"]["steps"]))
    assert deepest >= 21
    COVERAGE["limit15_deepest"] = deepest
    COVERAGE["limit15_most_steps"] = info["lit"]["steps"]
    return cases


# ---- limit7 ---------------------------------------------------------------------------------------------------------------------------------------------
def _cl_depth(lit, dist):
    hlit = max([257] + [s + 1 for s in range(286) if lit[s]])
    hdist = max([1] + [s + 1 for s in range(30) if dist[s]])
    chist = [0] * 19
    for s, _ in M.run_lengths(lit[:hlit] + dist[:hdist]):
        chist[s] += 1
    if sum(1 for f in chist if f) < 2:
        return 1, chist
    d = M.huffman_depths(chist)
    return max(d.values()), chist


def _limit7_start():
    """a start for the climb, laid out by hand: counts near 1, 2, 2, 3, 5, 9, 13, 21, 34, 56, 90 for the code-length symbols 18, 12, 1, 17, 11, 10, 0, 6, 7, 8, 9 -
    the heavy counts on the lengths that weigh least in the Kraft sum, which comes out at exactly 1; the two codes of one bit are the distance code"""
    want = {9: 90, 8: 56, 7: 34, 6: 21, 10: 9, 11: 5, 12: 2}
    assert sum(n << (15 - v) for v, n in want.items()) == K15
    left, seq = dict(want), []
    while any(left.values()):                                          # most left first, never four of a value in a row (a run of four would become a 16)
        v = max((v for v in left if left[v] and seq[-3:] != [v] * 3), key=lambda v: (left[v], v))
        seq.append(v)
        left[v] -= 1
    lit, at = [], 0
    gaps = [1] * 13 + [3, 7, 10] + [0] * 300
    for k, v in enumerate(seq):
        lit.append(v)
        if k % 12 == 5 and gaps[at]:                                   # the zeros: 13 single ones, three runs for a 17, and the rest in one run for the 18
            lit += [0] * gaps[at]
            at += 1
    assert at == 16
    head = lit[:40]
    lit = head + [0] * (286 - len(lit)) + lit[40:]
    assert len(lit) == 286 and lit[256]
    return lit, [1, 1] + [0] * 28


def _limit7_search(seed, rounds):
    """hill climbing over pairs of Kraft-complete length sets from the start above: split one code into two one bit longer, join two into one, or swap two
    places; the score is the unrestricted depth of the code-length code, then how uneven its counts are (the sum of squares leads across plateaus)"""
    rng = random.Random(seed)
    lit, dist = _limit7_start()
    score = lambda t: (t[0], sum(f * f for f in t[1]))           # noqa: E731
    first = _cl_depth(lit, dist)
    best = score(first)
    hits = {first[0]: (list(lit), list(dist))}
    simple = [0] * 286, [0] * 30                                   # the shallow end: a handful of codes
    simple[0][0] = simple[0][256] = simple[1][0] = simple[1][1] = 1
    hits.setdefault(_cl_depth(*simple)[0], simple)
    for _ in range(rounds):
        arr = lit if rng.random() < 0.8 else dist
        a, b = rng.randrange(len(arr)), rng.randrange(len(arr))
        old = (arr[a], arr[b])
        move = rng.random()
        if a == b:
            continue
        if move < 0.4 and 0 < arr[a] < 15 and arr[b] == 0:
            arr[a] = arr[b] = arr[a] + 1
        elif move < 0.7 and arr[a] == arr[b] and arr[a] > 1:
            arr[a], arr[b] = arr[a] - 1, 0
        elif move >= 0.7:
            arr[a], arr[b] = arr[b], arr[a]
        else:
            continue
        if lit[256] == 0:
            arr[a], arr[b] = old
            continue
        now = _cl_depth(lit, dist)
        if now[0] not in hits:
            hits[now[0]] = (list(lit), list(dist))
        if score(now) >= best:
            best = score(now)
        else:
            arr[a], arr[b] = old
    return hits


def _limit7():
    hits = _limit7_search(7007, 60000)
    deepest = max(hits)
    assert 7 in hits and 8 in hits and deepest >= 9, sorted(hits)
    cases = []
    for want in (7, 8, deepest):
        lit, dist = hits[want]
        hist = dyadic_hist(lit, dist)
        info = {}
        c = M.codes(hist, M.BLOCK, 0, info)
        assert c["lit_len"] == lit and c["dist_len"][:30] == dist and c["kind"] == 2 and len(c["cl"]) <= 316
        assert info["cl"]["depth"] == want and max(c["clen"]) == min(want, 7) and (info["cl"]["steps"] >= 1) == (want > 7), info["cl"]
        cases.append(_codes_case("limit7_depth_%d" % want, hist, depth=want, steps=info["cl"]["steps"]))
    COVERAGE["limit7_deepest"] = deepest
    return cases


# ---- rle ------------------------------------------------------------------------------------------------------------------------------------------------
def _rle_case(name, lit, dist, want_runs=(), synthetic_eob=False, **expect):
    assert synthetic_eob or lit[256], name
    hist = dyadic_hist(lit, dist)
    c = M.codes(hist, M.BLOCK, 0)
    assert c["kind"] == 2 and c["lit_len"] == lit, name
    if any(dist):
        assert c["dist_len"][:30] == dist, name
    have = runs(c["lit_len"][:c["hlit"]] + c["dist_len"][:c["hdist"]])
    for zero, k in want_runs:
        assert any((v == 0) == zero and r == k for v, r in have), (name, "no %s run of %d" % ("zero" if zero else "nonzero", k), have)
    for key, v in expect.items():
        assert c[key] == v, (name, key, c[key], v)
    return _codes_case(name, hist, **expect)


def _rle():
    cases = []
    nothing = [0] * 30
    # nonzero runs, the end of every cut of a 16: 1, 2, 3 (no 16), 4 (16 of 3), 6, 7 (16 of 6), 8, 9 (16 of 6 and single values), 10 (6 + 3), 13 (6 + 6)
    lit = _segments([(9, 13), (8, 10), (10, 9), (7, 8), (6, 7), (11, 6), (5, 4), (12, 3), (4, 2), (13, 1)], 286)
    fill_kraft(lit, list(range(256, 272)))
    cases.append(_rle_case("rle_nonzero_runs", lit, nothing, [(False, k) for k in (1, 2, 3, 4, 6, 7, 8, 9, 10, 13)], hlit=257 + sum(1 for v in lit[257:] if v), hdist=2))
    # zero runs around 3 and 11
    segs = []
    for z in (1, 2, 3, 10, 11, 12):
        segs += [(10, 1), (0, z)]
    lit = _segments(segs + [(10, 1)], 286)
    fill_kraft(lit, list(range(256, 272)))
    cases.append(_rle_case("rle_zero_runs_small", lit, nothing, [(True, k) for k in (1, 2, 3, 10, 11, 12)]))
    # zero runs around 138 and 138 + 11
    for z in (138, 139, 140, 141, 148, 149):
        lit = [0] * 286
        lit[z] = lit[z + 1] = 3
        fill_kraft(lit, [256] + list(range(z + 3, z + 17)))
        cases.append(_rle_case("rle_zero_run_%d" % z, lit, nothing, [(True, z)]))
    # 276 zeros from the literal/length lengths into the distance lengths: only a histogram without the end-of-block symbol has a zero at 256 (phase 2 alone)
    lit, dist = [0] * 286, [0] * 30
    lit[0] = lit[1] = 1
    dist[21] = dist[22] = 1
    cases.append(_rle_case("rle_zero_run_276_crossing", lit, dist, [(True, 276)], synthetic_eob=True, hlit=257, hdist=23))
    # a nonzero run that crosses: three 9s at the end of one alphabet, two at the start of the other; highest symbol 285, hdist 30
    lit = [0] * 286
    lit[283] = lit[284] = lit[285] = 9
    fill_kraft(lit, [256] + list(range(40, 54)))
    dist = [0] * 30
    dist[0] = dist[1] = 9
    dist[29] = 8
    fill_kraft(dist, list(range(3, 20)))
    cases.append(_rle_case("rle_nonzero_run_crossing", lit, dist, [(False, 5)], hlit=286, hdist=30))
    # highest used literal/length symbol 256, 257, 284, 285; hdist 2 (no distance: two codes of one bit; 1 cannot occur), 29, 30
    for top, hd in ((256, None), (257, 28), (284, 29), (285, None)):
        lit, dist = [0] * 286, [0] * 30
        lit[top] = 5
        fill_kraft(lit, [256] + list(range(97, 112)) if top != 256 else list(range(97, 112)))
        if hd is not None:
            dist[hd] = 4
            fill_kraft(dist, list(range(0, 15)))
        cases.append(_rle_case("rle_top_%d_hdist_%d" % (top, hd + 1 if hd is not None else 2), lit, dist, hlit=top + 1, hdist=hd + 1 if hd is not None else 2))
    # hclen: 19 needs a length of 15, 18 a length of 1 and none of 15; the smallest reachable is 12: a complete distance code of at most 30 symbols needs a
    # length of 4 or less (30 codes of 5 bits are not complete), and 4 stands in place 12 of the order, 3, 2 and 1 behind it
    lit, dist = [0] + [8] * 256 + [0] * 29, [4, 4] + [5] * 28
    cases.append(_rle_case("rle_hclen_12", lit, dist, hclen=12, hlit=257, hdist=30))
    lit = [0] * 286
    lit[65], lit[256] = 1, 15
    fill_kraft(lit, list(range(66, 80)))
    cases.append(_rle_case("rle_hclen_19", lit, nothing, hclen=19))
    lit = [0] * 286
    lit[65], lit[256] = 1, 14
    fill_kraft(lit, list(range(66, 80)))
    assert 15 not in lit
    cases.append(_rle_case("rle_hclen_18", lit, nothing, hclen=18))
    return cases


# ---- few ------------------------------------------------------------------------------------------------------------------------------------------------
def _few_codes():
    cases = []
    base = [0] * M.NHIST
    for s, f in ((65, 40), (66, 20), (67, 9), (256, 1)):
        base[s] = f
    for name, used in (("none", []), ("symbol_0", [0]), ("symbol_1", [1]), ("symbol_5", [5])):
        hist = list(base)
        for s in used:
            hist[M.NL + s], hist[257 + 2] = 7, 7
        c = M.codes(hist, 500, 0)
        second = 1 if used in ([], [0]) else 0                       # the partner of a lone symbol is symbol 0, of symbol 0 (or of nothing) symbol 1
        want = [0] * 30
        for s in used + [second] + ([0] if not used else []):
            want[s] = 1
        assert c["dist_len"] == want and c["kind"] == 2, (name, c["dist_len"])
        cases.append(_codes_case("few_distance_%s" % name, hist, n=500, hdist=max(used + [1]) + 1))
    for b in (0, 1, 255):
        hist = [0] * M.NHIST
        hist[b] = hist[256] = 1
        c = M.codes(hist, 1, zlib.crc32(bytes([b])))
        assert c["kind"] == 1
        cases.append(_codes_case("few_one_byte_%d" % b, hist, n=1, crc=zlib.crc32(bytes([b]))))
    # one literal alone with the end-of-block symbol, dynamic because n says so (phase 2 alone): bytes 0 and 1 as the lone literal
    for b in (0, 1, 255):
        hist = [0] * M.NHIST
        hist[b], hist[256] = 3000, 1
        c = M.codes(hist, 3000, 0)
        assert c["kind"] == 2 and sorted(s for s in range(286) if c["lit_len"][s]) == sorted([b, 256])
        cases.append(_codes_case("few_one_literal_%d" % b, hist, n=3000))
    return cases


# ---- store ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _store_texts():
    """texts of at most 64 bytes (one batch: no match, the histogram is the bytes') with dyn == n - 1, n, n + 1, by a seeded search"""
    rng = random.Random(2024)
    found = {}
    for _ in range(20000):
        n, k = rng.randrange(20, 65), rng.randrange(2, 40)
        text = bytes(rng.randrange(k) * 5 % 251 for _ in range(n))
        c = M.codes(M.histogram(list(text)), n, 0)
        if c["dyn"] - n in (-1, 0, 1) and c["dyn"] - n not in found:
            found[c["dyn"] - n] = text
            if len(found) == 3:
                break
    assert sorted(found) == [-1, 0, 1], sorted(found)
    out = []
    for d, text in sorted(found.items()):
        c = M.codes(M.histogram(list(text)), len(text), zlib.crc32(text))
        assert c["kind"] == (2 if d < 0 else 1), d
        out.append(("store_dyn_n%+d" % d, text))
    rng = random.Random(99)
    for n in (1, 2, 3, 4, 5, 255, 256, 257, 65279, 65280):
        text = bytes(rng.randrange(256) for _ in range(n))
        out.append(("store_n_%d" % n, text))
    return out


def _store_codes():
    cases = []
    for name, text in _store_texts():
        tokens, hist = M.match(text)
        crc = zlib.crc32(text)
        if name.startswith("store_n_"):
            assert M.codes(hist, len(text), crc)["kind"] == 1, name
        cases.append(_codes_case(name, hist, n=len(text), crc=crc))
    return cases


# ---- items (bits phase; the codes may be synthetic: the judge is the model's packer) -------------------------------------------------------------------
HEAD = [(0x8b1f, 16), (0x0408, 16), (0, 16), (0, 16), (0xff00, 16), (0x0006, 16), (0x4342, 16), (0x0002, 16)]


def _synthetic(pre, tokens, code, name):
    """a DefBlockCodes nothing but def_bits will read: the given items in front, the tokens under `code`, an end-of-block item, the padding, CRC and ISIZE"""
    nbits = sum(b for _, b in pre) + sum(M.token_item(t, code)[1] for t in tokens) + (code[256] >> 16)
    suf = [(code[256] & 0xffff, code[256] >> 16)] + ([(0, -nbits % 8)] if nbits % 8 else [])
    crc = zlib.crc32(name.encode())
    suf += [(crc & 0xffff, 16), (crc >> 16, 16), (len(tokens) & 0xffff, 16), (0, 16)]
    return dict(code=code, pre=pre, suf=suf, size=(nbits + 7) // 8 + 8, kind=2)


def _wide_code():
    """15 bits of ones for every symbol the wide tokens use: length symbol 284 (5 extra bits), distance symbol 29 (13 extra bits), and a few literals"""
    code = [0] * M.NHIST
    for s in (257 + 27, M.NL + 29, 256):
        code[s] = 0x7fff | 15 << 16
    for s, (v, b) in {65: (0, 1), 66: (1, 2), 67: (0x5, 3), 68: (0x1555, 13), 69: (0x7ffe, 15)}.items():
        code[s] = v | b << 16
    return code


def _items():
    cases = []
    code = _wide_code()
    wide = (257, 32768)                                             # extra values 30 of 5 bits and 8191 of 13 bits
    assert M.token_item(wide, code) == ((1 << 48) - 1 - (1 << 15), 48)
    for off in range(32):
        lead = [(((1 << off) - 1) & 0xffffff, off)] if off else []
        cases.append(dict(name="items_one_48_at_%d" % off, text=b"", tokens=[wide], codes=_synthetic(lead, [wide], code, "one%d" % off)))
        # 64 wide items behind a word and `off` bits: the window holds the carried word's `off` bits + 3072 bits, and the last item may reach a third word
        tokens = [wide] * 64 + [65]
        cases.append(dict(name="items_64x48_at_%d" % off, text=b"", tokens=tokens, codes=_synthetic([(0xabcdef, 32)] + lead, tokens, code, "full%d" % off)))
    COVERAGE["items_stage_words_needed"] = (31 + 64 * 48) // 32 + 1 + 1           # the carried word's bits + the batch, and the word the last item's high part may touch
    # batches that end exactly on a word, and batches that complete no word
    tokens = [65] * 32 + [66] * 16                                  # 32 x 1 bit + 16 x 2 bits = 64 bits
    cases.append(dict(name="items_batch_ends_on_word", text=b"", tokens=tokens, codes=_synthetic([(0xffffff, 24), (0xff, 8)], tokens, code, "word")))
    cases.append(dict(name="items_batches_of_no_word", text=b"", tokens=[65] * 5, codes=_synthetic([(5, 3)], [65] * 5, code, "noword")))
    rng = random.Random(31)
    code2 = list(code)
    code2[257 + 28], code2[M.NL] = 0x155 | 9 << 16, 1 | 1 << 16
    for n_pre in (64, 65, 128, 346):
        pre = [(rng.getrandbits(b), b) for b in (rng.randrange(1, 25) for _ in range(n_pre))]
        tokens = [rng.choice([65, 66, 67, 68, 69, wide, (258, 1)]) for _ in range(100)]
        cases.append(dict(name="items_n_pre_%d" % n_pre, text=b"", tokens=tokens, codes=_synthetic(pre, tokens, code2, "pre%d" % n_pre)))
    for nt in (63, 64, 65):
        tokens = [rng.choice([65, 66, 67, 68, 69, wide]) for _ in range(nt)]
        cases.append(dict(name="items_tokens_%d" % nt, text=b"", tokens=tokens, codes=_synthetic(HEAD[:3], tokens, code, "nt%d" % nt)))
    # what the synthetic cases reach, from the batches def_bits will form (64 header items, 64 tokens, the trailer: each batch a scan of its own)
    def batches(c):
        out, at = [], 0
        pre, tok = c["codes"]["pre"], [M.token_item(t, c["codes"]["code"]) for t in c["tokens"]]
        for group in [pre[k:k + 64] for k in range(0, len(pre), 64)] + [tok[k:k + 64] for k in range(0, len(tok), 64)] + [c["codes"]["suf"]]:
            out.append((at, [b for _, b in group]))
            at += sum(b for _, b in group)
        return out
    by_name = {c["name"]: batches(c) for c in cases}
    for off in range(32):
        assert any(at % 32 == off and w == [48] for at, w in by_name["items_one_48_at_%d" % off])
        assert any(at % 32 == off and w == [48] * 64 for at, w in by_name["items_64x48_at_%d" % off])
    assert any(sum(w) and (at + sum(w)) % 32 == 0 for at, w in by_name["items_batch_ends_on_word"])
    assert any(sum(w) and at // 32 == (at + sum(w)) // 32 for at, w in by_name["items_batches_of_no_word"])
    assert all(len(c["codes"]["pre"]) == n_pre for n_pre in (64, 65, 128, 346) for c in cases if c["name"] == "items_n_pre_%d" % n_pre)
    assert [len(c["tokens"]) for c in cases if c["name"].startswith("items_tokens_")] == [63, 64, 65]
    cases.append(_legal_wide())
    hist = _legal_widest()["hist"]
    tokens = []
    for s in range(256):
        tokens += [s] * hist[s]
    tokens = tokens[:100] + [wide] + tokens[100:] + [(3, M.DIST_BASE[s]) for s in range(30) for _ in range(hist[M.NL + s] - (s == 29))]
    assert M.histogram(tokens) == hist
    cases.append(dict(name="items_widest_legal_item", text=b"", tokens=tokens, codes=M.codes(hist, M.BLOCK, 0)))
    return cases


def _legal_wide():
    """a real histogram with 64 copies of the token (257, 32768) in one batch, their two symbols deep in their codes: both codes are chains of Fibonacci counts
    times 64 with the wide token's symbols at the bottom.  The block's 65 280 bytes pay for it: 64 x 257, three bytes for every other match (length 3, the
    heaviest literal/length symbol), and at least 32 768 literals in front, so that the distance exists."""
    best, fibs = None, _fib(40)
    for kd in range(2, 12):
        dist_counts = [64 * f for f in fibs[:kd]]                   # distance symbols 29 (the wide token's), 28, 27, ...
        short = sum(dist_counts) - 64
        left = M.BLOCK - 64 * 257 - 3 * short                       # bytes for literals
        if left < 32768:
            continue
        lit_counts, k = [], 1
        while sum(lit_counts) + 64 * fibs[k] <= left:
            lit_counts.append(64 * fibs[k])
            k += 1
        lit_counts[-1] += left - sum(lit_counts)
        hist = [0] * M.NHIST
        hist[257 + 27], hist[257], hist[256] = 64, short, 1
        for k, f in enumerate(lit_counts):
            hist[97 + k] = f
        for k, f in enumerate(dist_counts):
            hist[M.NL + 29 - k] = f
        c = M.codes(hist, M.BLOCK, 0)
        width = M.token_item((257, 32768), c["code"])[1]
        if c["kind"] == 2 and (best is None or width > best[0]):
            best = (width, hist, kd)
    width, hist, kd = best
    lits = []
    for s in range(256):
        lits += [s] * hist[s]
    random.Random(5).shuffle(lits)
    head = len(lits) // 64 * 64
    tokens = lits[:head] + [(257, 32768)] * 64 + lits[head:]
    for k in range(kd):
        tokens += [(3, M.DIST_BASE[29 - k])] * (hist[M.NL + 29 - k] - (64 if k == 0 else 0))
    assert M.histogram(tokens) == hist and head >= 32768
    text = M.expand(tokens)
    assert len(text) == M.BLOCK
    c = M.codes(hist, len(text), zlib.crc32(text))
    assert c["kind"] == 2
    widths = [M.token_item(t, c["code"])[1] for t in tokens]
    COVERAGE["items_fullest_legal_batch_bits"] = max(sum(widths[k:k + 64]) for k in range(0, len(widths), 64))
    assert COVERAGE["items_fullest_legal_batch_bits"] == 64 * width and width >= 18 + 2 * 8, width
    return dict(name="items_legal_wide_batch", text=text, tokens=tokens, codes=c)


@functools.lru_cache(maxsize=None)
def _legal_widest():
    """the widest item a legal code set gives: both of the wide token's symbols at 15 bits (two histograms of the limit15 kind) = 48 bits"""
    hist = [0] * M.NHIST
    for k, f in enumerate(_fib(17)):
        hist[[257 + 27, 256][k] if k < 2 else 95 + k] = f
        hist[M.NL + 29 - k] = f
    hist[257] = sum(_fib(17)) - 1                                    # every distance has a length: the other matches are of length 3
    c = M.codes(hist, M.BLOCK, 0)
    assert c["kind"] == 2 and M.token_item((257, 32768), c["code"])[1] == 48
    COVERAGE["items_widest_legal_item"] = 48
    return _codes_case("items_widest_legal_code_set", hist)


# ---- symbols --------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _symbols():
    """every length 3..258 and every distance symbol at its first and last distance, as a token list together with the text it expands to"""
    rng = random.Random(12)
    tokens = [rng.randrange(256) for _ in range(2000)]
    size = 2000
    pending = sorted(set(M.DIST_BASE + [M.DIST_BASE[s] + (1 << M.DIST_EXTRA[s]) - 1 for s in range(30)]))
    for length in list(range(3, 259)) + [3] * 60:
        ok = [d for d in pending if d <= size]
        if length == 3 and size > 32768 and not ok:
            break
        d = ok[0] if ok else 1 + rng.randrange(min(size, 300))
        if ok:
            pending.remove(d)
        tokens.append((length, d))
        size += length
        if rng.random() < 0.5:
            tokens.append(rng.randrange(256))
            size += 1
    assert not pending and size <= M.BLOCK
    text = M.expand(tokens)
    c = M.codes(M.histogram(tokens), len(text), zlib.crc32(text))
    assert c["kind"] == 2
    p = M.parse(M.bits(text, tokens, c))
    assert p["tokens"] == tokens and p["text"] == text
    seen_l, seen_d = set(), set()
    for t in p["tokens"]:
        if not isinstance(t, int):
            seen_l.add(M.len_symbol(t[0])), seen_d.add(M.dist_symbol(t[1]))
    for s in range(29):
        assert (s, M.LEN_EXTRA[s], 0) in seen_l and (s, M.LEN_EXTRA[s], (1 << M.LEN_EXTRA[s]) - 1 - (s == 27)) in seen_l, s      # (258 has its own symbol)
    for s in range(30):
        assert (s, M.DIST_EXTRA[s], 0) in seen_d and (s, M.DIST_EXTRA[s], (1 << M.DIST_EXTRA[s]) - 1) in seen_d, s
    assert {t[0] for t in tokens if not isinstance(t, int)} == set(range(3, 259))
    return dict(name="symbols_all", text=text, tokens=tokens, codes=c)


# ---- finder ---------------------------------------------------------------------------------------------------------------------------------------------
def _distinct(rng, n, low=0, high=256):
    """n bytes without a repeated 4-gram (a walk that never takes a 4-gram twice)"""
    out, seen = bytearray(), set()
    while len(out) < n:
        b = rng.randrange(low, high)
        if len(out) >= 3:
            g = bytes(out[-3:]) + bytes([b])
            if g in seen:
                continue
            seen.add(g)
        out.append(b)
    return bytes(out)


def _collision(rng):
    """two different 4-grams of capital letters with one hash"""
    seen = {}
    while True:
        g = bytes(rng.randrange(65, 91) for _ in range(4))
        h = M._hash(g, 0)
        if h in seen and seen[h] != g:
            return seen[h], g
        seen[h] = g


def _has(tokens, length=None, dist=None):
    return any(not isinstance(t, int) and (length is None or t[0] == length) and (dist is None or t[1] == dist) for t in tokens)


@functools.lru_cache(maxsize=None)
def _finder():
    rng = random.Random(404)
    out = []

    def add(name, text, check):
        tokens, _ = M.match(text)
        assert M.expand(tokens) == text and check(tokens), name
        out.append(("finder_" + name, text))

    a = _distinct(rng, 200, 97, 123)
    # a match that ends exactly at n; the same text cut so that a repeat has three bytes left: they are literals
    add("match_ends_at_n", a[:100] + a[10:30], lambda t: t[-1] == (20, 90))
    add("last_three_literals", a[:100] + a[10:30] + a[50:53], lambda t: t[-4:] == [(20, 90)] + list(a[50:53]))
    for n in (4, 5, 63, 64, 65, 67):
        add("n_%d" % n, (b"abcd" * 20)[:n], lambda t: all(isinstance(x, int) for x in t))
    for n in (68, 69, 131):
        add("n_%d" % n, (a[:64] * 3)[:n], lambda t, n=n: t[-1] == (n - 64, 64))
    # a match of 258 from lane 63 of batch 1: batches 2..5 have nothing to look up (cur >= base + 64)
    body = _distinct(rng, 700, 33, 127)
    text = body[:127] * 4 + body[400:460]                                # period 127: position 127 is the first that finds its 4-gram in an earlier batch
    add("258_from_lane_63", text, lambda t: t[127] == (258, 127) and all(isinstance(x, int) for x in t[:127]))
    add("back_to_back_258", b"G" * 64 + b"G" * (258 * 3 + 10), lambda t: t[64:67] == [(258, 1)] * 3)
    # a match back to position 0 (the table: distance = position)
    add("back_to_position_0", a[:64] + a[:40], lambda t: t[64] == (40, 64))
    # the last distance against the table.  A first match at distance 70 in batch 1 (70..99); from batch 2 on it is the last distance.  w stands at 101 (70
    # in front of 171) and at 114 (the table's entry in batch 2: the most recent one), each followed by another byte
    w = _distinct(rng, 12, 48, 58)
    tie = a[:70] + a[:30] + b"#" + w + b"<" + w + b">" + _distinct(rng, 44, 123, 200) + w + b"}" + _distinct(rng, 9, 200, 250)
    assert tie[101:113] == tie[114:126] == tie[171:183] == w
    add("last_distance_ties", tie, lambda t: t[70] == (30, 70) and _has(t, 12, 70) and not _has(t, None, 57))
    beat = tie[:119] + b"_" + tie[120:]                                  # the table's candidate shares 5 bytes, the last distance 12
    add("last_distance_longer", beat, lambda t: t[70] == (30, 70) and _has(t, 12, 70) and not _has(t, None, 57))
    lose = tie[:105] + b"^" + tie[106:]                                  # the place 70 back shares 4 bytes, the table's 12
    add("table_longer", lose, lambda t: t[70] == (30, 70) and _has(t, 12, 57) and not _has(t, 12, 70))
    # a table entry overwritten by a colliding later 4-gram: the repeat of the first is not found
    g1, g2 = _collision(rng)
    filler = _distinct(rng, 200, 97, 123)
    add("entry_overwritten", g1 + filler[:20] + g2 + filler[20:70] + g1 + filler[70:80], lambda t: all(isinstance(x, int) for x in t))
    add("entry_kept", g1 + filler[:20] + filler[90:94] + filler[20:70] + g1 + filler[70:80], lambda t: _has(t, 4))
    # a repeat whose only earlier occurrence is in the same batch: not found; one batch later: found
    add("repeat_in_same_batch", filler[:64] + filler[100:110] + filler[100:110] + filler[120:160], lambda t: all(isinstance(x, int) for x in t))
    add("repeat_one_batch_later", filler[:54] + filler[100:110] + filler[100:110] + filler[120:160], lambda t: _has(t, 10, 10))
    # distances 1, 63, 64 (32 768 and 32 769 are among the corner texts below)
    add("distance_1", b"ab" + b"Q" * 100, lambda t: _has(t, None, 1))
    add("distance_63", a[:63] * 3, lambda t: _has(t, None, 63))
    add("distance_64", a[:64] * 3, lambda t: _has(t, None, 64))
    got = {}
    for name, text in TC.corner_inputs():
        for k, at in enumerate(range(0, len(text), M.BLOCK)):
            piece = text[at:at + M.BLOCK]
            out.append(("corner_%s_%d" % (name, k), piece))
            if name.startswith("repeat_at_"):
                got[name] = M.match(piece)[0]
    assert _has(got["repeat_at_32768"], None, 32768) and not _has(got["repeat_at_32769"], None, 32769) and not _has(got["repeat_at_32769"], None, 32768)
    return out


def text_limit15_search(seeds=range(4), size=16000):
    """the attempt to reach the length limit from a TEXT: words of chosen lengths copied in Fibonacci proportions, so that the match lengths, not the literals,
    carry the skew (the finder swallows frequent literals).  -> (deepest unrestricted literal/length depth over the seeds, its text)"""
    best = (0, b"")
    for seed in seeds:
        rng = random.Random(seed)
        lengths = [4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51]
        words = [_distinct(rng, L, 97 + k, 98 + k + 6) for k, L in enumerate(lengths)]
        text = bytearray(b"".join(words))
        weights = list(reversed(_fib(len(words))))
        last = None
        while len(text) < size:
            k = rng.choices(range(len(words)), weights)[0]
            if k == last:
                continue
            text += words[k]
            last = k
        _, hist = M.match(bytes(text))
        info = {}
        M.codes(hist, len(text), 0, info)
        if info["lit"]["depth"] > best[0]:
            best = (info["lit"]["depth"], bytes(text))
    return best


# ---- what the tests take ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def codes_cases():
    cases = _limit15() + _limit7() + _rle() + _few_codes() + _store_codes() + [_legal_widest()]
    for b in bits_cases():
        if b["text"]:
            cases.append(_codes_case("codes_of_" + b["name"], M.histogram(b["tokens"]), n=len(b["text"]), crc=zlib.crc32(b["text"])))
    cases.append(_codes_case("eof_block", [0] * M.NHIST, n=0, crc=0))
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def bits_cases():
    cases = _items() + [_symbols()]
    # one literal and one match (the finder never gives this: the first batch has nothing to look up), and the stored blocks
    text = b"a" * 259
    tokens = [97, (258, 1)]
    cases.append(dict(name="few_one_literal_one_match", text=text, tokens=tokens, codes=M.codes(M.histogram(tokens), 259, zlib.crc32(text))))
    assert cases[-1]["codes"]["kind"] == 2 and M.expand(tokens) == text
    for name, text in _store_texts() + [("few_one_byte_%d" % b, bytes([b])) for b in (0, 1, 255)]:
        tokens, hist = M.match(text)
        cases.append(dict(name=name, text=text, tokens=tokens, codes=M.codes(hist, len(text), zlib.crc32(text))))
    cases.append(dict(name="eof_block", text=b"", tokens=[], codes=M.codes([0] * M.NHIST, 0, 0)))
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def match_texts():
    """(name, text): every text four times, its start at the four byte alignments (place() puts them there)"""
    base = _finder() + _store_texts() + [("few_one_byte_%d" % b, bytes([b])) for b in (0, 1, 255)] + [("symbols_text", _symbols()["text"])]
    # the attempt at the length limit from a text (bounded, seeded).  None reaches it: the text with the deepest tree is kept as a case all the same
    COVERAGE["text_limit15_deepest"], text = text_limit15_search()
    base.append(("text_limit15_attempt", text))
    out = []
    for name, text in base:
        if text:
            out += [("%s@%d" % (name, k), text) for k in range(4)]
    return out


def place(texts):
    """the texts in one buffer, the k-th at an offset of k mod 4 modulo 4 -> (bytes, offsets [len + 1] with the size as the last, sizes)"""
    buf, off = bytearray(), []
    for k, text in enumerate(texts):
        while len(buf) % 4 != k % 4:
            buf.append(0x5a)
        off.append(len(buf))
        buf += text
    return bytes(buf), off + [len(buf)], [len(t) for t in texts]


# ---- the batches of the three phase-level calls, with the model's answers (computed once) -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_of_text(text):
    tokens, hist = M.match(text)
    return tokens, hist, M.token_words(tokens)


@functools.lru_cache(maxsize=None)
def model_block(text):
    """the BGZF block of one text by the model's three phases (M.block, with the finder's result shared)"""
    tokens, hist, _ = model_of_text(text)
    out = M.bits(text, tokens, M.codes(hist, len(text), zlib.crc32(text)))
    assert len(out) == 18 + len(out[18:-8]) + 8 == (out[16] | out[17] << 8) + 1
    return out


@functools.lru_cache(maxsize=None)
def match_batch():
    import numpy as np
    names, texts = zip(*match_texts())
    buf, off, n = place(texts)
    assert sorted({o % 4 for o in off[:-1]}) == [0, 1, 2, 3]
    want = [model_of_text(t) for t in texts]
    return dict(names=names, texts=texts, text=buf, off=np.array(off, dtype=np.int64), n=np.array(n, dtype=np.uint32),
                nt=np.array([len(w[2]) for w in want], dtype=np.uint32), hist=np.array([w[1] for w in want], dtype=np.uint32),
                tok=[np.array(w[2], dtype=np.uint32) for w in want])


@functools.lru_cache(maxsize=None)
def codes_batch():
    import numpy as np
    cases = codes_cases()
    want = [M.codes_words(M.codes(c["hist"], c["n"], c["crc"])) for c in cases]
    return dict(names=[c["name"] for c in cases], hist=np.array([c["hist"] for c in cases], dtype=np.uint32), n=np.array([c["n"] for c in cases], dtype=np.uint32),
                crc=np.array([c["crc"] for c in cases], dtype=np.uint32), codes=np.array(want, dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def bits_batch():
    import numpy as np
    cases = bits_cases()
    buf, off, n = place([c["text"] for c in cases])
    return dict(names=[c["name"] for c in cases], text=buf, off=np.array(off, dtype=np.int64), n=np.array(n, dtype=np.uint32),
                nt=np.array([len(c["tokens"]) for c in cases], dtype=np.uint32), tok=[np.array(M.token_words(c["tokens"]), dtype=np.uint32) for c in cases],
                codes=np.array([M.codes_words(c["codes"]) for c in cases], dtype=np.uint32), want=[M.bits(c["text"], c["tokens"], c["codes"]) for c in cases])


def strided_tokens(tok):
    import numpy as np
    out = np.zeros((len(tok), M.BLOCK), dtype=np.uint32)
    for b, t in enumerate(tok):
        out[b, :t.size] = t
    return out


def write_case_file(path):
    """the three batches as tools/text_gz_host_test.cpp reads them (`cases FILE`): inputs, then what the model answers"""
    import numpy as np
    i64, u32 = (lambda *v: np.array(v, dtype="<i8").tobytes()), (lambda a: np.ascontiguousarray(a, dtype="<u4").tobytes())
    mb, cb, bb = match_batch(), codes_batch(), bits_batch()
    with open(path, "wb") as fh:
        fh.write(b"SVXDEFC1")
        fh.write(i64(0, mb["n"].size, len(mb["text"])) + mb["text"] + mb["off"].tobytes() + u32(mb["n"]) + u32(np.zeros(mb["n"].size)))
        fh.write(u32(mb["nt"]) + u32(mb["hist"]) + b"".join(u32(t) for t in mb["tok"]))
        fh.write(i64(1, cb["n"].size, 0) + np.zeros(cb["n"].size + 1, dtype="<i8").tobytes() + u32(cb["n"]) + u32(cb["crc"]) + u32(cb["hist"]) + u32(cb["codes"]))
        fh.write(i64(2, bb["n"].size, len(bb["text"])) + bb["text"] + bb["off"].tobytes() + u32(bb["n"]) + u32(np.zeros(bb["n"].size)))
        fh.write(u32(bb["nt"]) + b"".join(u32(t) for t in bb["tok"]) + u32(bb["codes"]) + u32([len(w) for w in bb["want"]]) + b"".join(bb["want"]))
    return mb["n"].size + cb["n"].size + bb["n"].size
