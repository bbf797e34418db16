"""The FASTA genome loader on the device (svx_genome_load_fasta, csrc/fasta.hip) against its specification, convert.genome_arrays: byte for byte, in the three
containers, with every line / record shape the specification answers."""
import os

import numpy as np
import pytest

import fasta_cases as F
import helpers as H
from svim_amd import _abi, _lib, convert

pytestmark = pytest.mark.gpu
KINDS = ("plain", "bgzf", "gzip")
KIND_IDS = ("plain", "blocks", "stream")            # (ids without the reader words of conftest.py: these tests belong to the first tier)


@pytest.fixture(scope="module")
def eng():
    return _lib.Engine(0)


def _check(eng, path, refs, kind=None):
    exp_off, exp_codes = convert.genome_arrays(path, refs)
    eng.set_genome(np.zeros(1, np.int64), np.full(1, 9, np.uint8))             # (whatever was resident is not what is compared)
    off, st = eng.load_genome_fasta(path, refs)
    got_off, got_codes = eng.fetch_genome()
    assert np.array_equal(off, exp_off) and np.array_equal(got_off, exp_off), (off, exp_off)
    assert got_codes.size == exp_codes.size
    if not np.array_equal(got_codes, exp_codes):
        k = int(np.nonzero(got_codes != exp_codes)[0][0])
        raise AssertionError("codes differ first at %d of %d: %r != %r" % (k, exp_codes.size, got_codes[k:k + 8], exp_codes[k:k + 8]))
    assert st["seq_bytes"] + st["dropped_bytes"] == st["raw_bytes"] and st["bases_kept"] == int(exp_off[-1]) and st["blank_bytes"] == 0
    if kind is not None:
        assert st["kind"] == kind
    return st


def test_fasta_golden_reference_gzip(eng):
    path = os.path.join(H.GOLDEN, "ref.fa.gz")
    st = _check(eng, path, H.REFS, "gzip")
    assert st["records_in_file"] == 3 and st["records_kept"] == 3 and st["bases_kept"] == 300000
    _check(eng, path, ["chr10", "chrX", "chr1"], "gzip")


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_fasta_line_and_record_shapes(eng, tmp_path, kind):
    for name, text, refs, cuts in F.small_cases():
        path = F.write(F.path_for(tmp_path, name, kind), text, kind, cuts)
        try:
            st = _check(eng, path, refs, kind)
        except AssertionError as e:
            raise AssertionError("%s (%s): %s" % (name, kind, e))
        assert st["raw_bytes"] == len(text), name
        assert st["records_in_file"] == sum(1 for l in text.split(b"\n") if l.startswith(b">")), name


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_fasta_staging_piece_boundaries(eng, tmp_path, kind):
    name, text, refs, cuts = F.piece_boundary_case()
    path = F.write(F.path_for(tmp_path, name, kind), text, kind, cuts)
    st = _check(eng, path, refs, kind)
    assert st["raw_bytes"] == len(text) > 2 * F.PIECE and st["records_kept"] == 3


def test_fasta_fetch_genome_after_set_genome(eng):
    off, codes = np.asarray([0, 3, 3, 8], np.int64), np.asarray([1, 2, 4, 8, 15, 0, 1, 2], np.uint8)
    eng.set_genome(off, codes)
    got_off, got_codes = eng.fetch_genome()
    assert np.array_equal(got_off, off) and np.array_equal(got_codes, codes)
    import torch
    d_off, d_codes = torch.from_numpy(off).cuda(), torch.from_numpy(codes).cuda()
    eng.set_genome(d_off, d_codes, on_device=True)                               # a borrowed device genome
    got_off, got_codes = eng.fetch_genome()
    assert np.array_equal(got_off, off) and np.array_equal(got_codes, codes)
    eng.set_genome(off, codes)


def test_fasta_symbols_outside_the_alphabet(eng, tmp_path):
    good, bad = F.record(b"good", F.bases(1, 500)), F.record(b"bad", F.bases(2, 100) + b"X*" + F.bases(3, 100))
    path = F.write(tmp_path / "bad.fa", good + bad, "plain")
    # in a requested record: the loader says which, load_genome raises what genome_arrays raises
    with pytest.raises(ValueError) as want:
        convert.genome_arrays(path, ["good", "bad"])
    with pytest.raises(_lib.FastaHostRoute) as e:
        eng.load_genome_fasta(path, ["good", "bad"])
    assert e.value.code == _abi.SVX_E_FASTA_SYMBOL and e.value.stats["bad_symbols"] == ["*", "X"]
    with pytest.raises(ValueError) as got:
        convert.load_genome(eng, path, ["good", "bad"])
    assert str(got.value) == str(want.value) and "'*', 'X'" in str(got.value)
    # in a record nobody asked for, and in the earlier of two records of one name: loads
    st = _check(eng, path, ["good"], "plain")
    assert st["records_in_file"] == 2 and st["records_kept"] == 1
    path = F.write(tmp_path / "bad_then_good.fa", bad + good + F.record(b"bad", F.bases(4, 77)), "plain")
    _check(eng, path, ["bad", "good"], "plain")
    for kind in ("bgzf", "gzip"):
        p = F.write(F.path_for(tmp_path, "bad", kind), good + bad, kind)
        with pytest.raises(_lib.FastaHostRoute) as e:
            eng.load_genome_fasta(p, ["bad"])
        assert e.value.code == _abi.SVX_E_FASTA_SYMBOL
        _check(eng, p, ["good"], kind)


def test_fasta_blanks_take_the_host_route(eng, tmp_path):
    for k, text in enumerate((b">a\nACGT \nACGT\n", b">a\nAC\tGT\n", b">a\n ACGT\n", b">a\nAC\rGT\n", b">a\nACGT\r\r\nAC\n")):
        path = F.write(tmp_path / ("blank%d.fa" % k), text, "plain")
        with pytest.raises(_lib.FastaHostRoute) as e:
            eng.load_genome_fasta(path, ["a"])
        assert e.value.code == _abi.SVX_E_FASTA_HOST and e.value.stats["host_reason"] == "blanks" and e.value.stats["blank_bytes"] > 0
        try:
            exp = convert.genome_arrays(path, ["a"])
        except ValueError as err:                                      # a blank inside a line is outside the alphabet
            with pytest.raises(ValueError) as got:
                convert.load_genome(eng, path, ["a"])
            assert str(got.value) == str(err)
            continue
        off, st = convert.load_genome(eng, path, ["a"])
        got_off, got_codes = eng.fetch_genome()
        assert st["route"] == "host" and np.array_equal(off, exp[0]) and np.array_equal(got_off, exp[0]) and np.array_equal(got_codes, exp[1])
    with pytest.raises(_lib.SvxError) as e:
        eng.load_genome_fasta(str(tmp_path / "missing.fa"), ["a"])
    assert "SVX_E_ARG" in str(e.value)


def test_fasta_over_budget_takes_the_host_route(eng, tmp_path, monkeypatch):
    text = F.record(b"a", F.bases(5, 3 << 20))
    path = F.write(tmp_path / "big.fa", text, "plain")
    monkeypatch.setenv("SVX_FASTA_BUDGET_MB", "4")
    with pytest.raises(_lib.FastaHostRoute) as e:
        eng.load_genome_fasta(path, ["a"])
    assert e.value.stats["host_reason"] == "budget"
    off, st = convert.load_genome(eng, path, ["a"])
    assert st["route"] == "host" and int(off[-1]) == 3 << 20
    monkeypatch.delenv("SVX_FASTA_BUDGET_MB")
    _check(eng, path, ["a"], "plain")


def test_fasta_256_mb_plain_equals_the_python_route(eng, tmp_path):
    path = str(tmp_path / "size.fa")
    n_per = (256 << 20) // 4 // 61 * 60
    with open(path, "wb") as fh:
        for k, nm in enumerate((b"s1", b"s2", b"s3", b"s4")):
            fh.write(b">" + nm + b" contig %d\n" % k)
            fh.write(F.lines_block(100 + k, n_per))
    refs = ["s3", "s1", "s4", "s2"]
    st = _check(eng, path, refs, "plain")
    assert st["raw_bytes"] == os.path.getsize(path) and st["bases_kept"] == 4 * n_per == st["seq_bytes"]
    assert st["records_in_file"] == 4 and st["records_kept"] == 4
    # two of the four: the bytes of the others are dropped
    st = _check(eng, path, ["s4", "s2"], "plain")
    assert st["bases_kept"] == 2 * n_per and st["seq_bytes"] == 4 * n_per


def test_fasta_dropin_clusters_same_on_both_routes(tmp_path, monkeypatch):
    """cluster_sv_signatures with the g_c1 options on tests/golden/ref.fa.gz: the device loader and SVX_GENOME_HOST=1 give the same clusters"""
    import svim_amd
    from svim_amd import SVIM_clustering
    o = H.options(H.load("g_c1.json.gz")["options"])
    assert o.genome.endswith("ref.fa.gz")
    g5 = H.load("g5_cluster.json.gz")
    case = max(g5["cases"], key=lambda c: sum(1 for r in c["signatures"] if r[0] == "INS"))
    assert sum(1 for r in case["signatures"] if r[0] == "INS") > 10

    def rows(res):
        return [[[c.contig, c.start, c.end, c.score, c.size, c.std_span, c.std_pos, len(c.members)] if k < 3 else
                 [c.source_contig, c.source_start, c.source_end, c.dest_contig, c.dest_start, c.dest_end, c.score, c.size, c.std_span, c.std_pos, len(c.members)]
                 for c in lst] for k, lst in enumerate(res)]
    out, genomes = {}, {}
    for route in ("device", "host"):
        if route == "host":
            monkeypatch.setenv("SVX_GENOME_HOST", "1")
        else:
            monkeypatch.delenv("SVX_GENOME_HOST", raising=False)
        SVIM_clustering._GENOMES.clear()
        seen = []
        orig = convert.load_genome

        def spy(*a, **kw):
            r = orig(*a, **kw)
            seen.append(r[-1]["route"])
            return r
        monkeypatch.setattr(convert, "load_genome", spy)
        out[route] = rows(svim_amd.cluster_sv_signatures([H.row_sig(r) for r in case["signatures"]], o))
        monkeypatch.setattr(convert, "load_genome", orig)
        assert seen == [route]
        genomes[route] = _lib.engine().fetch_genome()
    SVIM_clustering._GENOMES.clear()
    assert out["device"] == out["host"] and sum(len(x) for x in out["device"]) > 0
    assert np.array_equal(genomes["device"][0], genomes["host"][0]) and np.array_equal(genomes["device"][1], genomes["host"][1])
