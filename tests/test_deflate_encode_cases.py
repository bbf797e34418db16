"""The DEFLATE encoder (svim_amd/csrc/deflate_core.hpp), host build, held to its definition in plain Python (tests/deflate_model.py) phase by phase and end to
end on the directed cases of tests/deflate_encode_cases.py; the model's parser and zlib judge every block; one-step mutants of the header must differ from
the model on these cases (the method of DESIGN section 20).  The kernels: tests/test_gpu_deflate_encode_cases.py."""
import os
import shutil
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import deflate_encode_cases as DC
import deflate_model as M
import helpers as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "svim_amd", "csrc")
TOOL = os.path.join(REPO, "tools", "text_gz_host_test.cpp")


def check_match(got, mb):
    tok, nt, hist = got
    for b, name in enumerate(mb["names"]):
        assert nt[b] == mb["nt"][b] and np.array_equal(tok[b, :nt[b]], mb["tok"][b]), "%s: tokens (%d, the model has %d)" % (name, nt[b], mb["nt"][b])
        assert np.array_equal(hist[b], mb["hist"][b]), "%s: histogram" % name


def check_codes(got, cb):
    fields = (("code", 0, 320), ("pre", 320, 680), ("suf", 680, 688), ("n_pre, n_suf, size, kind", 688, 692))
    for b, name in enumerate(cb["names"]):
        for what, lo, hi in fields:
            assert np.array_equal(got[b, lo:hi], cb["codes"][b, lo:hi]), "%s: %s: %r, the model has %r" % (name, what, got[b, lo:hi].tolist(), cb["codes"][b, lo:hi].tolist())


def check_bits(got, bb):
    for b, name in enumerate(bb["names"]):
        want = bb["want"][b]
        have = got[b, :len(want)].tobytes()
        assert have == want, "%s: the block differs from the model's at byte %d of %d" % (name, next(i for i, (x, y) in enumerate(zip(have, want)) if x != y), len(want))
        assert not got[b, (len(want) + 3) // 4 * 4:].any(), "%s: bytes behind the block's last word" % name


def test_match_phase_equals_the_model():
    from svim_amd import _lib
    mb = DC.match_batch()
    check_match(_lib.text_gz_phase("match", mb["n"], mb["text"], mb["off"]), mb)


def test_codes_phase_equals_the_model():
    from svim_amd import _lib
    cb = DC.codes_batch()
    check_codes(_lib.text_gz_phase("codes", cb["n"], hist=cb["hist"], crc=cb["crc"]), cb)


def test_bits_phase_equals_the_model():
    from svim_amd import _lib
    bb = DC.bits_batch()
    check_bits(_lib.text_gz_phase("bits", bb["n"], bb["text"], bb["off"], tok=DC.strided_tokens(bb["tok"]), nt=bb["nt"], codes=bb["codes"]), bb)


def test_end_to_end_equals_the_model_and_parse_and_zlib_agree():
    """every text as one file: svx_text_gz_host = the model's block + the end-of-file block; the model's parser reads the block back to the tokens the model's
    finder made, every code complete (parse asserts Kraft = 1 for all three), and zlib inflates the payload to the same text"""
    from svim_amd import _lib
    kinds = set()
    for name, text in DC.match_texts():
        if not name.endswith("@0"):
            continue
        blk = DC.model_block(text)
        assert _lib.text_gz_host(text) == blk + M.EOF_BLOCK, name
        p = M.parse(blk)
        assert p["text"] == text == zlib.decompress(blk[18:-8], -15) and p["crc"] == zlib.crc32(text), name
        if p["kind"] == "dynamic":
            assert p["tokens"] == DC.model_of_text(text)[0], name
        kinds.add(p["kind"])
    assert kinds == {"stored", "dynamic"} and M.parse(M.EOF_BLOCK)["kind"] == "eof" and _lib.text_gz_host(b"") == M.EOF_BLOCK


def test_parse_and_zlib_read_the_blocks_of_the_bits_cases():
    """the blocks that come with their text (the synthetic code sets of `items` stand for no text: their judge is the packer): parse gives the token list the
    case was built from, with the width of every item, and zlib the text"""
    n = 0
    for c, blk in zip(DC.bits_cases(), DC.bits_batch()["want"]):
        if not c["text"]:
            continue
        p = M.parse(blk)
        assert p["text"] == c["text"] == zlib.decompress(blk[18:-8], -15), c["name"]
        if p["kind"] == "dynamic":
            assert p["tokens"] == c["tokens"] and p["widths"] == [M.token_item(t, c["codes"]["code"])[1] for t in c["tokens"]], c["name"]
            assert (p["hlit"], p["hdist"], p["hclen"], p["cl"], p["clen"]) == tuple(c["codes"][k] for k in ("hlit", "hdist", "hclen", "cl", "clen")), c["name"]
            assert p["pad"] == -c["codes"]["dyn_bits"] % 8
        n += 1
    assert n >= 18
    # the histograms of the codes phase as blocks of their own: the header alone, parsed (a histogram is no text, so the tokens are left out: end-of-block at once)
    for c in DC.codes_cases():
        k = M.codes(c["hist"], c["n"], c["crc"])
        if k["kind"] != 2 or not c["hist"][256]:
            continue
        p = M.parse(_header_only(k))
        assert (p["lit_len"], p["dist_len"]) == (k["lit_len"], k["dist_len"]) and p["cl"] == k["cl"], c["name"]
        assert zlib.decompress(_header_only(k)[18:-8], -15) == b"", c["name"]


def _header_only(k):
    """the dynamic header of a code set, the end-of-block code, padding: an empty block that both parsers must accept"""
    items = k["pre"][9:] + [k["suf"][0]]
    nbits = sum(b for _, b in items)
    items = items + ([(0, -nbits % 8)] if nbits % 8 else [])
    size = 18 + (nbits + 7) // 8 + 8
    return M.bits(b"", [], dict(kind=0, pre=k["pre"][:8] + [(size - 1, 16)] + items + [(0, 16)] * 4, suf=[]))


def test_coverage_figures():
    """what the families reached, as DESIGN section 33 records it (each family asserts its own edges when it is built)"""
    DC.codes_cases(), DC.bits_cases(), DC.match_texts()
    print(DC.COVERAGE)
    assert DC.COVERAGE == dict(limit15_deepest=21, limit15_most_steps=184, limit7_deepest=9, items_widest_legal_item=48, items_stage_words_needed=98,
                               items_fullest_legal_batch_bits=2240, text_limit15_deepest=11)
    assert DC.COVERAGE["items_stage_words_needed"] <= 112                    # DEF_STAGE


# ---- the mutant table -----------------------------------------------------------------------------------------------------------------------------------
# (the piece of deflate_core.hpp, which occurs exactly once; what stands there instead; None, or why no input tells the mutant from the original)
MUTANTS = [
    ("S.freq[S.sorted[li]] <= S.nfreq[ni]", "S.freq[S.sorted[li]] < S.nfreq[ni]", None),                        # a tie takes the leaf
    ("(g << 9 | t) < key", "(g << 9 | (nsym - t)) < (f << 9 | (nsym - s))", None),                              # ranked by (count, symbol)
    ("S.cnt[d < maxbits ? d : maxbits]++", "S.cnt[d <= maxbits ? d : maxbits]++", "at d == maxbits both arms are maxbits"),
    ("for (uint32_t i = maxbits - 1u; i > 0u; i--) if (S.cnt[i])", "for (uint32_t i = maxbits - 2u; i > 0u; i--) if (S.cnt[i])", None),
    ("if (used < 2u) S.freq[1] = 1u;", "if (used < 2u) S.freq[2] = 1u;", None),
    ("while (run >= 11u)", "while (run >= 12u)", None),
    ("run < 138u ? run : 138u", "run < 137u ? run : 137u", None),
    ("if (run >= 3u) {", "if (run >= 4u) {", None),
    ("while (run >= 3u) {", "while (run >= 4u) {", None),
    ("run < 6u ? run : 6u", "run < 5u ? run : 5u", None),
    ("while (hlit > 257u && !S.len[hlit - 1u]) hlit--;", "", None),
    ("while (hlit > 257u", "while (hlit > 256u", None),                                                         # (a histogram without the end-of-block symbol: phase 2 alone)
    ("while (hdist > 1u && !S.len[DEF_NL + hdist - 1u]) hdist--;", "", None),
    ("while (hdist > 1u", "while (hdist > 0u",
     "a distance code has at least two codes, on symbol 0 or 1 at the lowest (the rule for fewer than two used symbols), so the trim stops at 2 or above: the guard is never the reason"),
    ("while (hclen > 4u && !S.clen[order[hclen - 1u]]) hclen--;", "", None),
    ("while (hclen > 4u", "while (hclen > 3u",
     "the lengths always hold a nonzero value, and 8 - the first of them in the order - stands in place 5: the trim stops at 5 or above"),
    ("const bool stored = dyn >= n;", "const bool stored = dyn > n;", None),
    ("x = (s - 261u) >> 2;", "x = (s - 260u) >> 2;", None),
    ("if (s >= 265u && s < 285u)", "if (s >= 265u && s < 286u)", None),
    ("(s >= 4u ? (s >> 1) - 1u : 0u)", "(s >= 4u ? (s >> 1) : 0u)", None),
    ("const uint32_t pad = (uint32_t)((8u - (bits & 7u)) & 7u);", "const uint32_t pad = (uint32_t)(8u - (bits & 7u));", None),
    ("    if (l == 255u) return 28u;\n", "", None),
    ("const uint32_t nb = def_log2(d), e = nb - 1u;", "const uint32_t nb = def_log2(d), e = nb;", None),
    ("const uint32_t e = def_log2(l) - 2u;", "const uint32_t e = def_log2(l) - 1u;", None),
    ("if (l2 >= bl) { bl = l2; bd = rep; }", "if (l2 > bl) { bl = l2; bd = rep; }", None),
    ("rep != bd && ", "",
     "with rep == bd the second candidate is the first one over again: the same length, the same distance, so taking it changes nothing (the test saves the work)"),
    ("rep && rep <= p", "rep && rep < p",
     "rep is the distance of a match that began in an earlier batch at some m < p, and a distance never exceeds its position: rep <= m < p always"),
    ("p - (c - 1u) <= DEF_MAXDIST", "p - (c - 1u) < DEF_MAXDIST", None),
    ("if (p + 4u <= n) {", "if (p + 4u < n) {", None),
    ("if (look && p >= cur)", "if (look && p > cur)", None),
    ("if (bl < DEF_MINLEN) { bl = 0; bd = 0; }", "if (bl < DEF_MINLEN + 1u) { bl = 0; bd = 0; }", None),
    ("n - p < DEF_MAXLEN ? n - p : DEF_MAXLEN", "n - p < DEF_MAXLEN - 1u ? n - p : DEF_MAXLEN - 1u", None),
    ("(i == 256u ? 1u : 0u)", "0u", None),
    ("base + (uint32_t)D_LANE + 1u); }", "base + 1u); }", None),                                               # the most recent position of the batch enters the table
    ("const uint32_t hi_ = sh_ ? (uint32_t)(val_ >> (64u - sh_)) : 0u;", "const uint32_t hi_ = (uint32_t)(val_ >> ((64u - sh_) & 63u));", None),
    ("if (hi_) D_ATOMIC_OR(&L.stage[w_ + 2u], hi_);", "", None),
    ("i_ < done_ + 3u && i_ < DEF_STAGE", "i_ < done_ + 1u && i_ < DEF_STAGE",
     "a batch ends inside word done_ of the window, and the third word of an item is touched only by bits the item has: nothing is ever written behind word done_, so "
     "clearing up to it is enough (the two further words are a margin)"),
    ("i_ < done_ + 3u && i_ < DEF_STAGE; i_ += 64u) L.stage", "i_ < done_ && i_ < DEF_STAGE; i_ += 64u) L.stage", None),        # the carried word's old place stays set
    ("L.stage[i_] = i_ ? 0u : carry_;", "L.stage[i_] = 0u;", None),
    ("if (bp.bitpos & 31u) { D_LANE0 { dst[bp.wbase] = L.stage[0]; } }", "", None),
]
DIFFERENT = 3


def test_no_mutant_of_the_encoder_survives_unargued(tmp_path):
    """every entry of MUTANTS changes one place of deflate_core.hpp on a copy; tools/text_gz_host_test.cpp is built against the copy and run over the case file
    in a process of its own: it must end with status 3, "a block differs from the model" (a crash or a time limit is no detection).  The unchanged header goes
    the same way and must agree.  A mutant with a reason is one that no input can tell from the original: it must in fact agree on every case."""
    cases = str(tmp_path / "cases.bin")
    DC.write_case_file(cases)
    with open(os.path.join(CSRC, "deflate_core.hpp")) as fh:
        src = fh.read()

    def run_one(job):
        k, text = job
        d = str(tmp_path / ("m%d" % k))
        os.makedirs(d)
        with open(os.path.join(d, "deflate_core.hpp"), "w") as fh:
            fh.write(text)
        shutil.copy(os.path.join(CSRC, "textgz_phase.hpp"), d)
        exe = os.path.join(d, "tool")
        cc = subprocess.run(["g++", "-O1", "-w", "-std=c++17", "-DDEF_HOST", "-I", d, TOOL, "-lz", "-o", exe], capture_output=True, text=True)
        if cc.returncode:
            return k, "compile", cc.stderr[-1500:]
        try:
            run = subprocess.run([exe, "cases", cases], capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            return k, "time limit", ""
        return k, run.returncode, (run.stdout + run.stderr)[-600:]

    jobs = [(0, src)]
    for k, (piece, instead, _) in enumerate(MUTANTS, 1):
        assert src.count(piece) == 1 and instead != piece, "mutant %d: %r occurs %d times" % (k, piece, src.count(piece))
        jobs.append((k, src.replace(piece, instead)))
    with ThreadPoolExecutor(max_workers=min(8, H.granted_cpus())) as pool:
        results = sorted(pool.map(run_one, jobs), key=lambda r: r[0])
    assert results[0][1] == 0, "the unchanged header against the model: %r" % (results[0],)
    wrong = []
    for k, rc, out in results[1:]:
        piece, instead, reason = MUTANTS[k - 1]
        print("%2d  %-8s  %r -> %r" % (k, "killed" if rc == DIFFERENT else "equal" if rc == 0 else rc, piece.strip(), instead))
        if rc != (DIFFERENT if reason is None else 0):
            wrong.append("%d: %r -> %r: exit %r, %s %s" % (k, piece, instead, rc, "expected a difference" if reason is None else "argued to be equal", out.strip()[-300:]))
    assert not wrong, "%d of %d mutants:\n%s" % (len(wrong), len(MUTANTS), "\n".join(wrong))
    assert len(MUTANTS) == 40 and sum(1 for m in MUTANTS if m[2]) == 6


def test_phase_entries_are_exported_and_refuse_what_a_phase_would_index_out_of_range_with():
    """svx_text_gz_phase / svx_text_gz_phase_host stand in the symbol list; csrc/textgz_phase.hpp turns away, before either build runs, an item of 49 bits, a
    code of 16 bits, a literal token of 256, a match token with stray bits, more tokens than a block has bytes, a block that overflows its slot, a histogram
    that counts more tokens than a block has bytes, a text outside the buffer"""
    import pytest
    from svim_amd import _lib
    for name in ("svx_text_gz_phase", "svx_text_gz_phase_host"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    good = dict(code=[1 | 1 << 16] * M.NHIST, pre=[(5, 3)], suf=[(0, 5)], size=1, kind=2)
    words = lambda **kw: np.array([M.codes_words(dict(good, **kw))], dtype=np.uint32)      # noqa: E731
    tok = np.zeros((1, M.BLOCK), dtype=np.uint32)
    call = lambda codes, tok=tok, nt=1, n=0: _lib.text_gz_phase("bits", [n], b"", [0, 0], tok=tok, nt=[nt], codes=codes)      # noqa: E731
    assert call(words()).shape == (1, 65536)
    wide = np.full((1, M.BLOCK), 0x80000000 | 32767 << 9 | 254, dtype=np.uint32)
    stray = tok.copy()
    stray[0, 0] = 0x81000000
    lit256 = tok.copy()
    lit256[0, 0] = 256
    for bad in (dict(codes=words(pre=[(0, 49)])), dict(codes=words(code=[1 | 16 << 16] * M.NHIST)), dict(codes=words(), tok=lit256), dict(codes=words(), tok=stray),
                dict(codes=words(), nt=M.BLOCK + 1), dict(codes=words(code=[0x7fff | 15 << 16] * M.NHIST), tok=wide, nt=M.BLOCK), dict(codes=words(kind=3)),
                dict(codes=words(kind=1), n=5)):
        with pytest.raises(_lib.SvxError, match="SVX_E_ARG"):
            call(**bad)
    hist = np.zeros((1, M.NHIST), dtype=np.uint32)
    hist[0, 65] = M.BLOCK + 2
    with pytest.raises(_lib.SvxError, match="SVX_E_ARG"):
        _lib.text_gz_phase("codes", [100], hist=hist, crc=[0])
    with pytest.raises(_lib.SvxError, match="SVX_E_ARG"):
        _lib.text_gz_phase("match", [0], b"", [0, 0])
