"""Both DEFLATE decoders (svim_amd/csrc/inflate_core.hpp: one wave per block; inflate_lanes.hpp: one lane per block), built for the host, on streams that zlib's
COMPRESSOR never writes and zlib's DECOMPRESSOR answers (tests/deflate_streams.py): distances up to 32 768, one block over a whole BGZF payload, empty blocks
in mid-stream, length 258 as symbol 284 + 31, headers without a distance code, 15-bit codes ..., and every rule of RFC 1951 broken once on purpose.  zlib's
verdict is the reference for each stream: its bytes for a sound one, its refusal for the others."""
import collections
import os
import subprocess
import zlib

import pytest

import deflate_streams as DS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I", os.path.join(REPO, "svim_amd", "csrc")]
WAVE_SRC = os.path.join(REPO, "tools", "inflate_host_test.cpp")
LANES_SRC = os.path.join(REPO, "tools", "inflate_lanes_host_test.cpp")
GIVEN_UP = os.path.join(REPO, "tests", "golden", "deflate_lanes_given_up.tsv")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]

# what sections 2 and 3 of the corpus must hold, by group
GROUPS = ["distances", "lengths", "block structure", "code tables", "input geometry", "other encoders", "invalid: block type", "invalid: stored",
          "invalid: header counts", "invalid: code-length code", "invalid: code lengths", "invalid: literal/length set", "invalid: distance set", "invalid: symbols",
          "invalid: distance too far", "invalid: no distance code", "invalid: truncated", "invalid: declared size"]
# the seams of the wave decoder and the streams built to go through them (counter of tools/inflate_host_test.cpp --corpus -> names)
SEAMS = {
    "walk": ["table/litlen-max-length-11", "table/litlen-max-length-15", "table/dist-max-length-9", "table/dist-max-length-15", "table/end-of-block-is-the-longest-code",
             "table/15-bit-code-then-1-bit-code", "input/body-of-15-bit-codes"],
    "far": ["dist/4095-sym285", "dist/4096-sym285", "dist/4097-sym284x31", "dist/32506-sym285", "dist/32507-sym285", "dist/32768-sym284x31", "dist/32768-source-at-offset-0",
            "dist/source-from-global-memory-into-the-ring", "dist/ring-around-flush-pending-1039", "block/matches-back-into-stored-fixed-dynamic-predecessors"],
    "fence": ["dist/4096-sym285", "dist/32768-source-at-offset-0", "dist/source-from-global-memory-into-the-ring", "dist/ring-around-flush-pending-1040"],
    "flush": ["dist/ring-around-flush-pending-1038", "dist/ring-around-flush-pending-1039", "dist/ring-around-flush-pending-1040", "len/match-across-every-multiple-of-1024"],
    "stepcap": ["len/chain-of-258-to-65536-dist-1", "len/chain-of-258-to-65536-dist-300"],
    "wide2": ["input/multi-window-steps-literals-and-short-matches"], "wide3": ["input/multi-window-steps-literals-and-short-matches"],
    "wide4": ["input/multi-window-steps-literals-and-short-matches", "input/multi-window-steps-literals-and-short-matches.fixed"],
}
# ... and the streams that must NOT take the canonical walk: their longest code is exactly as long as the one-lookup tables (10 / 8 bits)
NO_WALK = ["table/litlen-max-length-9", "table/litlen-max-length-10", "table/dist-max-length-8"]


def _zlib(data):
    try:
        return zlib.decompress(data, -15)
    except zlib.error:
        return DS.INVALID


def test_constructed_streams_are_what_zlib_says_they_are():
    """Before any decoder of ours sees a stream: a sound one inflates, under zlib, to the payload its tokens stand for; one that breaks a rule is refused by zlib
    (a lying declared size: zlib's byte count differs from it).  The labels of the corpus are zlib's verdicts, not ours."""
    corpus = DS.corpus()
    names = [c[0] for c in corpus]
    assert len(set(names)) == len(names) and 150 <= len(corpus) <= 600
    per_group = collections.Counter()
    for name, group, data, expected, size in corpus:
        per_group[group] += 1
        got = _zlib(data)
        if expected == DS.INVALID:
            assert group.startswith("invalid"), name
            if group == "invalid: declared size":
                assert got != DS.INVALID and abs(len(got) - size) == 1, name
            else:
                assert got == DS.INVALID, "%s: zlib accepts it (%d bytes)" % (name, len(got))
        else:
            assert got == expected and len(expected) == size <= 65536, name
    print("\ncorpus: %d streams, %.1f MB of payload" % (len(corpus), sum(len(c[3]) for c in corpus if c[3] != DS.INVALID) / 1e6))
    for g in GROUPS:
        print("  %-32s %d" % (g, per_group[g]))
        assert per_group[g] > 0, g
    assert set(per_group) == set(GROUPS)
    assert sum(len(c[2]) for c in corpus) < 8 << 20


def test_constructor_helpers():
    """the pieces the corpus is made of, each against its definition"""
    for n in range(3, 259):
        ls, x = DS.length_symbol(n)
        assert DS.LEN_BASE[ls] + x == n and 0 <= x < (1 << DS.LEN_EXTRA[ls]) or (n == 258 and ls == 28)
    for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 24, 25, 4096, 4097, 24576, 24577, 32768):
        ds, x = DS.dist_symbol(d)
        assert DS.DIST_BASE[ds] + x == d and 0 <= x < (1 << DS.DIST_EXTRA[ds])
    freqs = [1 << k for k in range(40)] + [0, 0, 3]                           # a Huffman tree far deeper than 15: the limit must hold and the code stay complete
    for limit in (7, 9, 15):
        lens = DS.huffman_lengths(freqs, limit)
        assert max(lens) <= limit and DS.kraft(lens, limit) == 1 << limit and lens[40] == 0 and all(lens[:40])
    for m in (3, 7, 9, 10, 11, 15):
        lens = DS.skewed(m)([5] * 20 + [0] * 10 + [1] * 8 if m > 4 else [1, 2, 3, 4, 5])
        assert max(lens) == m and DS.kraft(lens) == 1 << 15
    assert sorted(set(DS.flat_lengths([1] * 286))) == [8, 9] and sorted(set(DS.flat_lengths([1] * 30))) == [4, 5]
    seq = [0] * 150 + [5] * 9 + [0] * 4 + [7]
    for flags in ((True, True, True), (False, False, True), (True, False, False), (False, False, False)):
        items = DS.rle_items(seq, *flags)
        back = []
        for s, x in items:
            back += [s] if s < 16 else ([back[-1]] * (3 + x) if s == 16 else [0] * ((3 if s == 17 else 11) + x))
            assert s < 16 or flags[s - 16]
        assert back == seq
    # a stream of each block type, and the same tokens through the three policies
    payload = DS.rand_bytes(5, 3000, b"ACGT") * 3
    for pol in DS.POLICIES.values():
        assert zlib.decompress(pol(payload), -15) == payload
    assert zlib.decompress(DS.policy_one_block(b""), -15) == b"" and zlib.decompress(DS.policy_short_blocks(b""), -15) == b""


def _build(out, src, flags):
    return subprocess.run(["g++", "-std=c++17", *flags, *INC, src, "-lz", "-o", out], capture_output=True, text=True)


@pytest.fixture(scope="module")
def corpus_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("deflate_corpus") / "corpus.bin")
    DS.write_corpus_file(path, DS.corpus())
    return path


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory, corpus_file):
    """{decoder: {name: (verdict, {counter: value})}} from the two host builds"""
    d = tmp_path_factory.mktemp("deflate_tools")
    out = {}
    for key, src, flags in (("wave", WAVE_SRC, ["-O2", "-DINF_HOST"]), ("lanes", LANES_SRC, ["-O2"])):
        exe = str(d / key)
        b = _build(exe, src, flags)
        assert b.returncode == 0, b.stderr[-2000:]
        run = subprocess.run([exe, "--corpus", corpus_file], capture_output=True, text=True, timeout=600)
        assert run.returncode in (0, 1), (run.stdout[-500:], run.stderr[-2000:])
        table = {}
        for line in run.stdout.splitlines():
            f = line.split("\t")
            if len(f) >= 2:
                w = f[2].split() if len(f) > 2 else []
                table[f[0]] = (f[1], {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)})
        assert set(table) == {c[0] for c in DS.corpus()}, run.stdout[-500:]
        out[key] = table
    return out


def test_sanitizer_builds_on_the_corpus(tmp_path, corpus_file):
    """The whole corpus - the rule-breaking streams above all - through both host builds under AddressSanitizer + UndefinedBehaviorSanitizer, every stream at eight
    alignments: no report, no byte outside the output (the tools keep guard bytes around it).  tests/test_gpu_deflate_streams.py sends a rule-breaking stream to
    the GPU only from this same corpus: this test is the gate for that."""
    for key, src, flags in (("wave", WAVE_SRC, ["-DINF_HOST"]), ("lanes", LANES_SRC, [])):
        exe = str(tmp_path / (key + "_asan"))
        b = _build(exe, src, SANITIZE + flags)
        if b.returncode != 0 and "sanitize" in b.stderr:
            pytest.skip("no sanitizer runtime in this toolchain")
        assert b.returncode == 0, b.stderr[-2000:]
        run = subprocess.run([exe, "--corpus", corpus_file], capture_output=True, text=True, timeout=900)
        assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, (key, run.stdout[-600:], run.stderr[-3000:])
        assert "%d streams, 0 wrong" % len(DS.corpus()) in run.stdout


def test_wave_decoder_answers_every_stream_like_zlib(verdicts):
    wrong = {}
    for name, group, data, expected, size in DS.corpus():
        v = verdicts["wave"][name][0]
        if expected == DS.INVALID:
            if not (v.startswith("refused -") and -8 <= int(v.split()[1]) <= -1) and not (group == "invalid: declared size" and v.startswith("refused ")):
                wrong[name] = v
        elif v != "equal":
            wrong[name] = v
    assert not wrong, wrong


def test_lane_decoder_answers_or_gives_up_and_what_it_gives_up_is_pinned(verdicts):
    """A lane may hand a block back to the wave-per-block decoder (stored blocks, tables beyond its share of LDS, anything it refuses); what it answers is zlib's
    bytes, and it answers no stream that breaks a rule.  The set it hands back (with the site in inflate_lanes.hpp that did) is part of its behaviour: a changed
    rule shows here.  tests/golden/deflate_lanes_given_up.tsv: <name> TAB <site>."""
    wrong, given_up = {}, {}
    for name, group, data, expected, size in DS.corpus():
        v = verdicts["lanes"][name][0]
        if v.startswith("given up "):
            given_up[name] = int(v.split()[2])
        elif v != "equal" or expected == DS.INVALID:
            wrong[name] = v
    assert not wrong, wrong
    with open(GIVEN_UP) as fh:
        pinned = {l.split("\t")[0]: int(l.split("\t")[1]) for l in fh.read().splitlines() if l}
    assert given_up == pinned, sorted(set(given_up.items()) ^ set(pinned.items()))
    decoded = [c[0] for c in DS.corpus() if c[3] != DS.INVALID and c[0] not in given_up]
    print("\nlane decoder: %d streams decoded, %d given up (by site: %s)" % (len(decoded), len(given_up), dict(collections.Counter(given_up.values()))))
    # plain fixed-Huffman blocks and stored blocks are outside what a lane handles; the far distances, both spellings of length 258, a block without a distance
    # code and a single one-bit distance code are inside
    assert given_up["dist/32768-sym285"] == 8 and given_up["block/stored-65535"] == 7
    for name in ("dist/32768.small-alphabet", "dist/4096.small-alphabet", "dist/1.small-alphabet", "len/every-symbol-min-max-extra.small-alphabet",
                 "table/hdist-1-with-length-0-no-distance-code", "table/single-distance-code-of-1-bit-used-by-matches", "len/chain-of-258-to-65536-dist-1"):
        assert name in decoded, name


def test_the_streams_reach_the_seams_they_were_built_for(verdicts):
    """Counters of the host build (INF_SEAM, multi-window steps): canonical walks for codes beyond the one-lookup tables - and none when the longest code just
    fits them -, match sources read back from global memory and the fence in front of them, input refills, flushes, steps cut at the step cap, multi-window steps
    of every width.  A stream that does not reach its seam is a bug of the test."""
    wave = verdicts["wave"]
    print()
    for counter, names in sorted(SEAMS.items()):
        for name in names:
            assert wave[name][1][counter] > 0, (counter, name, wave[name][1])
        hit = sorted(n for n, (v, c) in wave.items() if c.get(counter, 0) > 0)
        print("  %-8s %3d streams, e.g. %s" % (counter, len(hit), ", ".join(hit[:3])))
    for name in NO_WALK:
        assert wave[name][1]["walk"] == 0, name
    assert wave["input/body-of-15-bit-codes"][1]["refill"] >= 8 * 50                   # ~56 KiB of input, a KiB per refill, eight alignments
    assert wave["input/body-of-15-bit-codes"][1]["walk"] >= 8 * 30000
