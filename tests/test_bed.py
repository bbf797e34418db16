"""The BED / signature-VCF text without a GPU: the Python definition (candidates.get_bed_entr*, SVIM_COMBINE.write_candidates_python, the *_python signature
writers, the five as_string forms) against what the reference wrote (tests/golden/g_bed_cases.json.gz), the table builders of the device route, the ABI."""
import ctypes as C
import os
import re
import subprocess

import bed_cases as BC
from svim_amd import SVIM_CLUSTER, SVIM_COMBINE, _abi, _lib, bed, candidates as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(directory, names):
    out = []
    for n in names:
        with open(os.path.join(directory, n)) as fh:
            out.append(fh.read())
    return out


def test_member_text_of_every_signature_class():
    G = BC.load()
    sigs = BC.signatures(G)
    assert {t for t, _ in G["sigs"]} == set(BC.SIG_CLASSES)
    for s, (bar, tab) in zip(sigs, G["as_string"]):
        assert s.as_string("|") == bar and s.as_string() == tab


def test_python_definition_equals_the_reference_case_by_case(tmp_path):
    G = BC.load()
    sigs = BC.signatures(G)
    assert [c["name"] for c in G["cases"] if c["python_only"]] == ["int_score"]
    for case in G["cases"]:
        clusters, cands = BC.cluster_lists(G, case, sigs), BC.candidate_lists(G, case, sigs)
        for slot, objs in zip(G["cluster_slots"], clusters):
            for o, want in zip(objs, case["cluster_entries"][slot]):
                got = [o.get_bed_entry()] if hasattr(o, "contig") else list(o.get_bed_entries())
                assert got == want["bed"] and o.get_vcf_entry() == want["vcf"], (case["name"], slot)
        for slot, objs in zip(G["candidate_slots"], cands):
            for o, want in zip(objs, case["candidate_entries"][slot]):
                got = [o.get_bed_entry()] if slot in ("DEL", "INV", "INS") else list(o.get_bed_entries())
                assert got == want, (case["name"], slot)
        assert SVIM_CLUSTER.signature_bed_texts_python(clusters) == case["sig_beds"], case["name"]
        assert SVIM_CLUSTER.vcf_header_text(G["version"]) + SVIM_CLUSTER.signature_vcf_body_python(clusters) == case["sig_vcf"], case["name"]
        assert SVIM_COMBINE.candidate_bed_texts_python(cands) == case["cand_beds"], case["name"]
        d = tmp_path / case["name"]
        d.mkdir()
        SVIM_CLUSTER.write_signature_clusters_bed_python(str(d), clusters)
        SVIM_CLUSTER.write_signature_clusters_vcf_python(str(d), clusters, G["version"])
        SVIM_COMBINE.write_candidates_python(str(d), cands)
        assert _read(str(d / "signatures"), G["sig_bed_files"]) == case["sig_beds"]
        assert _read(str(d / "signatures"), ["all.vcf"]) == [case["sig_vcf"]]
        assert _read(str(d / "candidates"), G["cand_bed_files"]) == case["cand_beds"]
    assert [n for n, _, _ in SVIM_CLUSTER._BED_FILES] == G["sig_bed_files"] and [n for n, _, _ in SVIM_COMBINE._CANDIDATE_BED_FILES] == G["cand_bed_files"]


def test_golden_holds_what_the_issue_asks_for():
    G = BC.load()
    main = [c for c in G["cases"] if c["name"] == "main"][0]
    text = "".join(main["sig_beds"]) + main["sig_vcf"] + "".join(main["cand_beds"])
    for needle in ("None", ";0.0;", "0.30000000000000004", "0.6666666666666666", "origin potentially deleted", "3500000000", "left_fwd", "left_rev", "right_fwd", "right_rev",
                   ";all;", "chr01", "chr10", "INS;cigar", "BND;suppl", "DUP_TAN;suppl;3"):
        assert needle in text, needle
    digits = {len(re.sub(r"[^0-9]", "", repr(x)).strip("0")) for c in G["cases"] for slot in c["clusters"].values() for _, a in slot for x in a if isinstance(x, float)}
    assert {1, 2, 16, 17} <= digits
    scores = [c for c in G["cases"] if c["name"] == "scores"][0]
    assert len(scores["clusters"]["DEL"]) >= 80 and any(a[3] != round(a[3]) for _, a in scores["clusters"]["DEL"])
    body = [l for l in main["sig_vcf"].split("\n") if l and not l.startswith("#")]
    keys = [(l.split("\t")[0], int(l.split("\t")[1])) for l in body]
    assert keys == sorted(keys) and [k[0] for k in keys] != sorted((k[0] for k in keys), key=lambda n: (len(n), n))      # string order, not the natural one
    same = [l.split("\t")[4] for l in body if l.startswith("chr1\t101\t") and ";END=200;" in l]
    assert same[:4] == ["<DEL>", "<DEL>", "<INS>", "<INS>"] or same[0] == "<DEL>" and same.index("<INS>") < same.index("<INV>") < same.index("<DUP:TANDEM>")
    empty = [c for c in G["cases"] if c["name"] == "empty"][0]
    assert set(empty["sig_beds"]) == {""} and set(empty["cand_beds"]) == {""}


def test_table_builders_say_what_fits():
    G = BC.load()
    sigs = BC.signatures(G)
    for case in G["cases"]:
        clusters, cands = BC.cluster_lists(G, case, sigs), BC.candidate_lists(G, case, sigs)
        ct, ca = bed.cluster_table_from_lists(clusters), bed.candidate_table_from_lists(cands)
        if case["python_only"]:
            assert ct is None and ca is None, case["name"]
            continue
        table, names, sig, reads = ct
        assert table.n == sum(len(x) for x in clusters) and list(table.type_count) == [len(clusters[k]) for k in (0, 1, 2, 3, 5, 4)]
        assert sig.n == len({id(m) for lst in clusters for c in lst for m in c.members}) and set(names) <= set(G["contigs"])
        table, names, sig, reads = ca
        assert table.n == sum(len(x) for x in cands) and list(table.class_count) == [len(cands[k]) for k in (3, 1, 0, 2, 4, 5)]
    # what else a table cannot say
    s = sigs[0]
    d = K.CandidateDeletion("chr1", 5, 50, [s], 1.0, None, None)
    assert bed.candidate_table_from_lists(([], [], [], [d], [], [])) is not None
    for change in (dict(score=5), dict(score=float("nan")), dict(std_span=3), dict(std_pos=float("nan")), dict(source_end=1 << 31), dict(source_contig=7)):
        c = K.CandidateDeletion("chr1", 5, 50, [s], 1.0, None, None)
        for k, v in change.items():
            setattr(c, k, v)
        assert bed.candidate_table_from_lists(([], [], [], [c], [], [])) is None, change
    odd = BC.SIG_CLASSES["DEL"]("chr1", 1, 2, "split", "r")
    assert bed.candidate_table_from_lists(([], [], [], [K.CandidateDeletion("chr1", 5, 50, [odd], 1.0, None, None)], [], [])) is None


def test_abi_structs_match_the_header(tmp_path):
    src = tmp_path / "abi.c"
    fields = {"svx_bed_inputs": _abi.BedInputs, "svx_bed_stats": _abi.BedStats}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "svx.h"', "int main(void) {"]
    for name, st in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f, _ in st._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    lines.append('printf("products %d %d %d %d\\n", SVX_BED_SIGNATURE_BEDS, SVX_BED_SIGNATURE_VCF, SVX_BED_CANDIDATE_BEDS, SVX_BED_MAX_FILES);')
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).splitlines()
    got = dict(l.split() for l in out[:-1])
    for name, st in fields.items():
        assert int(got[name]) == C.sizeof(st), name
        for f, _ in st._fields_:
            assert int(got["%s.%s" % (name, f)]) == getattr(st, f).offset, (name, f)
    assert out[-1].split()[1:] == [str(x) for x in (_abi.BED_SIGNATURE_BEDS, _abi.BED_SIGNATURE_VCF, _abi.BED_CANDIDATE_BEDS, _abi.BED_MAX_FILES)]
    for s in ("svx_bed", "svx_bed_set_read_names", "svx_bed_count", "svx_bed_fetch", "svx_bed_get_stats", "svx_format_repr", "svx_format_repr_many",
              "svx_format_repr_device"):
        assert s in _lib.SYMBOLS and getattr(_lib.lib(), s)


def test_drop_in_names():
    import svim_amd
    assert svim_amd.SVIM_COMBINE.write_candidates is SVIM_COMBINE.write_candidates
    for f in (SVIM_CLUSTER.write_signature_clusters_bed, SVIM_CLUSTER.write_signature_clusters_vcf, SVIM_COMBINE.write_candidates):
        assert f.__code__.co_varnames[:2] == ("working_dir", "clusters") or f.__code__.co_varnames[:2] == ("working_dir", "candidates")
