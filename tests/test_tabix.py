"""The tabix index without a GPU: the definition (svim_amd/tabix.py) held to its own structure and to a brute-force scan through region queries; the host
build of csrc/textindex_core.hpp (svx_text_index_host; the kernels write the same bytes, tests/test_gpu_text_index.py holds them to that) byte for byte
against the definition; the refusals; the position order of the VCF lines against the reference's own bodies; the host build under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import text_gz_cases as TC
import text_index_cases as XC
import vcf_cases as VC
from svim_amd import tabix

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "svim_amd", "csrc")


@pytest.fixture(scope="module")
def big():
    """(name, preset, text, stream, coff, uoff, header bytes in front, index bytes) of the two large texts; the VCF one lies behind a compressed header"""
    from svim_amd import harness
    out = []
    for name, preset, text, head in (("seeded_vcf", XC.VCF, TC.seeded_vcf_text(), b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"),
                                     ("seeded_bed", XC.BED, XC.seeded_bed_text(), b"")):
        stream, coff, uoff = XC.tables(text)
        zhead = harness.bgzf_blocks(head)
        out.append((name, preset, text, zhead + stream, coff, uoff, len(zhead), tabix.build_index(text, coff, uoff, preset, len(zhead))))
    return out


def test_the_seeded_texts_are_what_the_issue_says(big):
    vcf = big[0][2]
    assert len(vcf) > 6_000_000 and vcf.count(b"\n") == 6000 and len({l.split(b"\t")[0] for l in vcf.splitlines()}) == 8
    assert XC.python_status(vcf, XC.VCF) == 0 and XC.python_status(big[1][2], XC.BED) == 0
    assert max(len(l) for l in vcf.splitlines()) < XC.BLOCK


def test_structure(big):
    for name, preset, text, _, coff, uoff, base, ix in big:
        parsed = XC.check_structure(ix, text, coff, uoff, preset, base)
        assert len(parsed["names"]) == (8 if preset == XC.VCF else 6), name
        assert sum(len(c) for b in parsed["bins"] for c in b.values()) > 1000, name


def test_reg2bin_and_reg2bins():
    rng = np.random.default_rng(3)
    assert tabix.reg2bin(0, 1) == 4681 and tabix.reg2bin(0, 1 << 29) == 0 and tabix.reg2bin((1 << 29) - 1, 1 << 29) == 37448
    assert tabix.reg2bin(16383, 16385) == 585 and tabix.reg2bin(1 << 26, (1 << 26) + 1) == 4681 + 4096 and tabix.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0
    for _ in range(3000):
        beg = int(rng.integers(0, (1 << 29) - 1))
        end = min(1 << 29, beg + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 29)))))
        b = tabix.reg2bin(beg, end)
        # a query that touches the record names the record's bin
        q = int(rng.integers(beg, end))
        assert b in tabix.reg2bins(q, q + 1) and b in tabix.reg2bins(beg, end)


def _regions(text, preset, rng, n_random):
    recs = [tabix.parse_line(l, preset) for l in text.split(b"\n")]
    recs = [r for r in recs if r is not None]
    names = sorted({r[0] for r in recs})
    regions = [(r[0], r[1], r[2]) for r in recs]                                            # every record's own interval
    top = max(r[2] for r in recs)
    for k in range(1, top // 16384 + 2, max(1, top // 16384 // 150)):                      # windows at multiples of 16 384 +- 1
        for c in names[:2]:
            regions += [(c, 16384 * k - 1, 16384 * k), (c, 16384 * k, 16384 * k + 1), (c, 16384 * k - 1, 16384 * k + 1), (c, 16384 * (k - 1), 16384 * k)]
    regions += [(c, 0, 1 << 29) for c in names] + [(b"chrNONE", 0, 1 << 29), (names[0], top + 5, top + 900), (names[0], 10, 10)]
    random = []
    for _ in range(n_random):
        beg = int(rng.integers(0, top + 20000))
        random.append((names[int(rng.integers(0, len(names)))], beg, beg + 1 + int(rng.integers(0, 1 << int(rng.integers(2, 17))))))
    return regions, random


def test_queries_equal_brute_force(big):
    rng = np.random.default_rng(2026)
    for name, preset, text, bgzf, coff, uoff, base, ix in big:
        parsed = tabix.parse_index(ix)
        regions, random = _regions(text, preset, rng, 2000)
        lines = text.split(b"\n")
        recs = [(l, tabix.parse_line(l, preset)) for l in lines]
        recs = [(l, r) for l, r in recs if r is not None]
        by_contig = {}
        for l, r in recs:
            by_contig.setdefault(r[0], []).append((r[1], r[2], l))

        def brute(c, beg, end):
            return [l for b, e, l in by_contig.get(c, ()) if end > beg and b < end and e > beg]
        assert brute(*regions[0]) == tabix.brute_force(text, preset, *regions[0])          # (the fast scan is the slow one)
        n_blocks = len(coff) - 1
        for c, beg, end in regions:
            assert tabix.query(parsed, bgzf, c, beg, end) == brute(c, beg, end), (name, c, beg, end)
        empty = full = 0
        for c, beg, end in random:
            stats = {}
            got = tabix.query(parsed, bgzf, c, beg, end, stats)
            assert got == brute(c, beg, end), (name, c, beg, end)
            empty += not got
            full += bool(got)
            assert stats.get("blocks", 0) <= max(3, n_blocks // 4), (name, c, beg, end, stats)      # only the blocks the chunks name, not the file
        print("%s: %d random regions, %d empty answers, %d not" % (name, len(random), empty, full))
        assert empty >= len(random) // 4 and full >= len(random) // 4, (name, empty, full)


def test_host_build_equals_the_definition(big):
    from svim_amd import _lib
    for name, preset, text, _, coff, uoff, base, ix in big:
        assert _lib.text_index_host(text, coff, uoff, preset, base) == ix, name
    for name, preset, text in XC.corner_texts():
        stream, coff, uoff = XC.tables(text)
        want = tabix.build_index(text, coff, uoff, preset, 77)
        assert _lib.text_index_host(text, coff, uoff, preset, 77) == want, name
        if tabix.records(text, coff, uoff, preset):
            XC.check_structure(want, text, coff, uoff, preset, 77)
        else:
            assert tabix.parse_index(want)["names"] == [] and len(want) == 44
    by_name = {n: (p, t) for n, p, t in XC.corner_texts()}
    p, t = by_name["long_line"]
    recs = tabix.records(t, *XC.tables(t)[1:], p)
    assert [(r[1], r[2]) for r in recs] == [(99, 900), (1999, 70000), (1999, 2000), (4, 6)]          # an END= behind the parsed head of a line is not seen
    assert recs[1][4] >> 16 > recs[1][3] >> 16 and recs[2][4] >> 16 > recs[2][3] >> 16                # the long lines cross blocks
    p, t = by_name["line_ends_at_block_edge"]
    stream, coff, uoff = XC.tables(t)
    recs = tabix.records(t, coff, uoff, p)
    assert recs[1][3] == coff[1] << 16 and recs[0][4] == recs[1][3]                                   # the second line is the new block's offset 0
    p, t = by_name["spans_level_0"]
    assert tabix.reg2bin(*tabix.parse_line(t.split(b"\n")[0], p)[1:]) == 0
    p, t = by_name["end_before_pos"]
    assert [tabix.parse_line(l, p)[1:] for l in t.split(b"\n")[:2]] == [(4999, 5004), (4999, 5000)]
    p, t = by_name["end_at_2_29"]
    assert tabix.parse_line(t, p)[2] == 1 << 29 and len(tabix.parse_index(tabix.build_index(t, *XC.tables(t)[1:], p))["linear"][0]) == 32768


def test_refusals():
    from svim_amd import _lib
    for name, preset, text, code in XC.refused_texts():
        stream, coff, uoff = XC.tables(text)
        for build in (tabix.build_index, _lib.text_index_host):
            with pytest.raises(tabix.TabixError) as e:
                build(text, coff, uoff, preset, 0)
            assert e.value.code == code, (name, build)
    # the reference's own order: POS drops inside a contig, and contigs with one natural key interleave
    G = VC.load()
    n = 0
    for case in G["cases"]:
        body = case["body"]
        if not body:
            continue
        pairs = [(l.split("\t")[0], int(l.split("\t")[1])) for l in body]
        drops = sum(1 for a, b in zip(pairs, pairs[1:]) if a[0] == b[0] and b[1] < a[1])
        runs = 1 + sum(1 for a, b in zip(pairs, pairs[1:]) if a[0] != b[0])
        text = "".join(l + "\n" for l in body).encode()
        stream, coff, uoff = XC.tables(text)
        if len(body) == 42:                                                              # every full body: the file tabix refuses
            assert 1 <= drops <= 3 and runs == 14 and len({p[0] for p in pairs}) == 8, (case["name"], drops, runs)
            n += 1
        elif drops == 0 and runs == len({p[0] for p in pairs}):                          # (a body of one class can be in order by chance)
            assert _lib.text_index_host(text, coff, uoff, XC.VCF, 0) == tabix.build_index(text, coff, uoff, XC.VCF, 0)
            continue
        for build in (tabix.build_index, _lib.text_index_host):
            with pytest.raises(tabix.TabixError) as e:
                build(text, coff, uoff, XC.VCF, 0)
            assert e.value.code == tabix.E_ORDER, case["name"]
    assert n >= 8


def test_position_order_of_the_vcf_body():
    from svim_amd import SVIM_COMBINE, _lib
    G = VC.load()
    ref = SVIM_COMBINE.GenomeText(G["genome"])
    n = 0
    for case in G["cases"]:
        o = VC.options(case)
        objs = VC.objects(VC.case_rows(G, case), G["sigs"])
        args = (*VC.lists6(objs), case["types"], o, not o.symbolic_alleles, ref)
        assert SVIM_COMBINE.vcf_body_python(*args) == case["body"] == SVIM_COMBINE.vcf_body_python(*args, position_order=False, contig_names=G["contigs"])
        body = SVIM_COMBINE.vcf_body_python(*args, position_order=True, contig_names=G["contigs"])
        assert sorted(body) == sorted(case["body"]), case["name"]                       # the same lines, ids included
        assert {l.split("\t")[2] for l in body} == {l.split("\t")[2] for l in case["body"]} and len({l.split("\t")[2] for l in body}) == len(body)
        pairs = [(l.split("\t")[0], int(l.split("\t")[1])) for l in body]
        assert 1 + sum(1 for a, b in zip(pairs, pairs[1:]) if a[0] != b[0]) == len({p[0] for p in pairs}) or not body, case["name"]
        assert all(b[1] >= a[1] for a, b in zip(pairs, pairs[1:]) if a[0] == b[0]), case["name"]
        # ties keep the reference's order
        at = {l: k for k, l in enumerate(case["body"])}
        assert all(at[a] < at[b] for a, b, pa, pb in zip(body, body[1:], pairs, pairs[1:]) if pa == pb), case["name"]
        if body:
            text = "".join(l + "\n" for l in body).encode()
            stream, coff, uoff = XC.tables(text)
            assert _lib.text_index_host(text, coff, uoff, XC.VCF, 0) == tabix.build_index(text, coff, uoff, XC.VCF, 0)
            n += 1
    assert n >= 10


def test_host_build_under_the_sanitizers(tmp_path):
    """tools/text_index_host_test.cpp with textindex_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer over a seeded fuzz of sorted, unsorted,
    truncated and garbage texts on uneven block tables: every call ends in an index that walks back to its size or in one of the two refusals, no report"""
    out = str(tmp_path / "text_index_host_asan")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC,
                            os.path.join(REPO, "tools", "text_index_host_test.cpp"), os.path.join(CSRC, "textindex_host.cpp"), "-o", out], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("no sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([out, "fuzz", "7", "3000"], capture_output=True, text=True, timeout=1200)
    assert run.returncode == 0 and "3000 texts" in run.stdout and " 0 malformed" in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    indexed, order, rng = (int(run.stdout.split(w)[0].split()[-1]) for w in (" indexed", " out of order", " out of range"))
    assert indexed > 1000 and order > 300 and rng > 100, run.stdout[-300:]


def test_symbols_declared_and_exported():
    import ctypes as C
    from svim_amd import _abi, _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "svx.h")).read()
    for name in ("svx_text_index", "svx_text_index_count", "svx_text_index_fetch", "svx_text_index_get_stats", "svx_text_index_host", "svx_vcf_position_order"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert C.sizeof(_abi.TextIndexStats) == 17 * 8 and (_abi.SVX_E_ORDER, _abi.SVX_E_RANGE) == (tabix.E_ORDER, tabix.E_RANGE) == (-9, -10)
    assert "#define SVX_E_ORDER        (-9)" in header and "#define SVX_E_RANGE        (-10)" in header
