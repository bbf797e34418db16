"""The VCF text without a GPU: the Python definition of a line (svim_amd.candidates, SVIM_COMBINE.vcf_body_python) against what the reference wrote
(tests/golden/g_vcf_cases.json.gz), the natural contig order, and the host form of the device's STD_* formatter."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import vcf_cases as VC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G():
    return VC.load()


def test_entry_methods_match_the_reference(G):
    from svim_amd import SVIM_COMBINE
    ref = SVIM_COMBINE.GenomeText(G["genome"])
    n = 0
    for case in G["cases"]:
        sw = case["switches"]
        objs = VC.objects(VC.case_rows(G, case), G["sigs"])
        seq, rz = not sw["symbolic_alleles"], (sw["read_names"], sw["zmws"])
        for name, per_cand in case["entries"].items():
            assert len(per_cand) == len(objs[name])
            for c, methods in zip(objs[name], per_cand):
                for m, text in methods.items():
                    if m.endswith("_as_dup") or name == "BND":
                        got = getattr(c, m)(*rz)
                    elif name == "INS":
                        got = c.get_vcf_entry(seq, ref, sw["insertion_sequences"], *rz)
                    else:
                        got = getattr(c, m)(seq, ref, *rz)
                    assert got == text, (case["name"], name, m)
                    n += 1
    assert n > 1000


def test_entry_methods_take_the_reference_keywords(G):
    objs = VC.objects(G["rows"], G["sigs"])
    c = objs["INS"][0]
    assert c.get_vcf_entry(insertion_sequences=True, read_names=True) == c.get_vcf_entry(False, None, True, True, False)
    assert objs["BND"][0].get_vcf_entry(zmws=True) == objs["BND"][0].get_vcf_entry(False, True)
    with pytest.raises(TypeError):
        objs["BND"][0].get_vcf_entry(sequence_alleles=True)
    with pytest.raises(TypeError):
        objs["DEL"][0].get_vcf_entry(False, None, False, False, False)


def test_body_and_header_match_the_reference(G):
    from svim_amd import SVIM_COMBINE
    ref = SVIM_COMBINE.GenomeText(G["genome"])
    for case in G["cases"]:
        o = VC.options(case)
        objs = VC.objects(VC.case_rows(G, case), G["sigs"])
        body = SVIM_COMBINE.vcf_body_python(*VC.lists6(objs), case["types"], o, not o.symbolic_alleles, ref)
        assert body == case["body"], case["name"]
        header = SVIM_COMBINE.vcf_header("2.0.0", G["contigs"], [len(G["genome"][c]) for c in G["contigs"]], case["types"], o)
        assert [l for l in header if not l.startswith("##fileDate=")] == case["header"], case["name"]
    assert not [c for c in G["cases"] if c["name"] == "mask_none"][0]["body"]


def test_natural_order_and_ranks(G):
    from svim_amd import SVIM_COMBINE, convert
    names = G["natural"]["names"]
    assert [e[0][0] for e in SVIM_COMBINE.sorted_nicely([((n, 0, 0), "", "DEL") for n in names])] == G["natural"]["sorted"]
    rank = convert.natural_ranks(names)
    by_rank = sorted(range(len(names)), key=lambda i: rank[i])           # stable: equal ranks keep the input order, as the reference's sort keeps them
    assert [names[i] for i in by_rank] == G["natural"]["sorted"]
    r = dict(zip(names, rank.tolist()))
    assert r["chr1"] == r["chr01"] == r["chr001"] and r["chr2"] < r["chr10"] and r["1"] < r["chr1"]
    assert len(set(rank.tolist())) == len(set(tuple(convert.natural_key(n)) for n in names))


def test_zmw_ids():
    from svim_amd import convert
    ids = convert.zmw_ids(["m1/100/0_500", "m1/100/600_900", "m1/1000/ccs", "readA", "a/b/c/d", "m1/100/x"]).tolist()
    assert ids[0] == ids[1] == ids[5] and ids[2] not in (ids[0], -1) and ids[3] == ids[4] == -1


def test_format_std_is_pythons_round(G):
    from svim_amd import _lib
    for x, text in G["std"]:
        assert _lib.vcf_format_std(x) == text
    assert _lib.vcf_format_std(float("nan")) == "." and _lib.vcf_format_std(-0.0) == "."
    L = _lib.lib()
    out = C.create_string_buffer(32)
    rng = random.Random(77)
    xs = []
    for _ in range(50_000):
        xs.append(10.0 ** rng.uniform(-9, 9))
        k = rng.randrange(1, 10 ** rng.randrange(1, 13))
        x = k / 1000.0
        if x < 1e9:
            xs += [x, np.nextafter(x, 0.0), np.nextafter(x, np.inf)]
    xs += [0.125, 0.375, 2.5e-3, 7.5e-3, 1e-9, 4.9e-324, 999999999.995, 9999999999.0, 0.045, 1.005, 1.015, 1.025]
    assert len(xs) >= 190_000
    for x in xs:
        x = float(x)
        assert L.svx_vcf_format_std(C.c_double(x), out) == 0
        assert out.value.decode() == str(round(x, 2)), x
    for bad in (1e10, 3e300, float("inf"), -1e12):
        with pytest.raises(_lib.SvxError):
            _lib.vcf_format_std(bad)


def test_symbols_declared_and_exported():
    from svim_amd import _abi, _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "svx.h")).read()
    for name in ("svx_vcf", "svx_vcf_count", "svx_vcf_fetch", "svx_vcf_get_stats", "svx_vcf_format_std"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert C.sizeof(_abi.VcfParams) == 28 and C.sizeof(_abi.VcfStats) == 7 * 8 + 4 * 8 + 6 * 8 + 5 * 8
