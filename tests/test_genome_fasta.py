"""The FASTA genome loader, the parts that need no GPU: the ABI constants, the container probe, the step from the header table to the placement
(svx_fasta_plan) and the route switch of convert.load_genome.  The device passes are tested in test_gpu_genome_fasta.py."""
import gzip
import os
import re

import numpy as np
import pytest

import fasta_cases as F
from svim_amd import _abi, _lib, convert


def _header_table(text):
    """what the device passes hand to svx_fasta_plan, restated on the host: (blob, hdr_pos, hdr_rank) of every '>' in the first column"""
    pos, rank, kept, in_hdr = [], [], 0, False
    at = 0
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            pos.append(at)
            rank.append(kept)
            in_hdr = True
        else:
            in_hdr = False
        if not in_hdr:
            kept += len(line.replace(b"\r", b""))
        at += len(line) + 1
    blob = b"".join((text[p + 1:p + 1 + F.NAME_BYTES]).ljust(F.NAME_BYTES, b"\0") for p in pos)
    return blob, np.asarray(pos, dtype=np.int64), np.asarray(rank + [kept], dtype=np.int64)


def test_fasta_abi_constants_and_version():
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "svx.h")).read()
    d = dict(re.findall(r"#define (SVX_FASTA_[A-Z_]+|SVX_E_FASTA_[A-Z]+)\s+\(?(-?[0-9< ]+)\)?", header))
    assert eval(d["SVX_FASTA_TILE"]) == _abi.FASTA_TILE and eval(d["SVX_FASTA_PIECE"]) == _abi.FASTA_PIECE
    assert eval(d["SVX_FASTA_NAME_BYTES"]) == _abi.FASTA_NAME_BYTES
    assert int(d["SVX_E_FASTA_SYMBOL"]) == _abi.SVX_E_FASTA_SYMBOL and int(d["SVX_E_FASTA_HOST"]) == _abi.SVX_E_FASTA_HOST
    assert _abi.ERRORS[_abi.SVX_E_FASTA_SYMBOL] == "SVX_E_FASTA_SYMBOL" and _abi.ERRORS[_abi.SVX_E_FASTA_HOST] == "SVX_E_FASTA_HOST"
    assert {"svx_genome_load_fasta", "svx_genome_fetch", "svx_fasta_probe", "svx_fasta_plan"} <= set(_lib.SYMBOLS)
    assert _lib.lib().svx_version() >= 101


def test_fasta_probe_tells_the_containers_apart(tmp_path):
    text = F.record(b"a", F.bases(1, 200000)) + F.record(b"b", F.bases(2, 10))
    p = F.write(tmp_path / "x.fa", text, "plain")
    assert _lib.fasta_probe(p) == ("plain", len(text), 0)
    p = F.write(tmp_path / "x.bgzf.fa.gz", text, "bgzf", cuts=[5, 100])
    kind, raw, nb = _lib.fasta_probe(p)
    n_data = 2 + -(-(len(text) - 100) // 0xff00)
    assert (kind, raw, nb) == ("bgzf", len(text), n_data + 1)                 # with the empty block at the end
    assert gzip.open(p, "rb").read() == text                                     # the test's block writer writes what gzip readers take
    p = F.write(tmp_path / "x.gzip.fa.gz", text, "gzip")
    assert _lib.fasta_probe(p) == ("gzip", -1, 0)
    # BGZF blocks followed by an ordinary gzip member: not BGZF as a whole
    with open(tmp_path / "mixed.fa.gz", "wb") as fh:
        fh.write(F.bgzf_bytes(text[:1000], eof=False) + gzip.compress(text[1000:]))
    assert _lib.fasta_probe(str(tmp_path / "mixed.fa.gz"))[0] == "gzip"
    # a block cut short
    with open(tmp_path / "cut.fa.gz", "wb") as fh:
        fh.write(F.bgzf_bytes(text)[:-40])
    assert _lib.fasta_probe(str(tmp_path / "cut.fa.gz"))[0] == "gzip"
    open(tmp_path / "empty.fa", "wb").close()
    assert _lib.fasta_probe(str(tmp_path / "empty.fa")) == ("plain", 0, 0)
    with pytest.raises(_lib.SvxError):
        _lib.fasta_probe(str(tmp_path / "missing.fa"))


@pytest.mark.parametrize("case", [c for c in F.small_cases() if b" \n" not in c[1]], ids=lambda c: c[0])
def test_fasta_plan_places_records_like_genome_arrays(case, tmp_path):
    name, text, refs, _ = case
    path = F.write(tmp_path / "c.fa", text, "plain")
    exp_off, _ = convert.genome_arrays(path, refs)
    blob, pos, rank = _header_table(text)
    dest, off, kept = _lib.fasta_plan(blob, pos, rank, len(text), refs)
    assert np.array_equal(off, exp_off)
    # every placed record starts at its contig's offset; the placed lengths fill the contigs
    placed = sorted((int(d), int(rank[h + 1] - rank[h])) for h, d in enumerate(dest) if d >= 0)
    assert kept == len(placed) and sum(l for _, l in placed) == int(off[-1])
    assert all(d in set(off[:-1].tolist()) for d, _ in placed)


def test_fasta_plan_last_record_of_a_name_wins_and_order_follows_references():
    text = b">d one\nAAAA\n>e\nCC\n>d two\nGGGGGG\n>f\nT\n"
    blob, pos, rank = _header_table(text)
    dest, off, kept = _lib.fasta_plan(blob, pos, rank, len(text), ["f", "absent", "d"])
    assert dest.tolist() == [-1, -1, 1, 0] and off.tolist() == [0, 1, 1, 7] and kept == 2
    dest, off, kept = _lib.fasta_plan(blob, pos, rank, len(text), [])
    assert dest.tolist() == [-1] * 4 and off.tolist() == [0] and kept == 0
    # no header at all
    dest, off, kept = _lib.fasta_plan(b"", [], [8], 10, ["a"])
    assert dest.size == 0 and off.tolist() == [0, 0]


def test_fasta_plan_leaves_odd_names_to_the_host():
    for text, refs in ((b">\nAC\n", ["a"]), (b"> a\nAC\n", ["a"]), (b">caf\xc3\xa9\nAC\n", ["a"]), (b">" + b"n" * F.NAME_BYTES + b" d\nAC\n", ["a"]),
                       (b">a\nAC\n", ["a", "a"])):
        blob, pos, rank = _header_table(text)
        with pytest.raises(_lib.FastaHostRoute):
            _lib.fasta_plan(blob, pos, rank, len(text), refs)
    # the longest name the blob holds, and a name that ends with the file
    for text in (b">" + b"n" * (F.NAME_BYTES - 1) + b"\nACG\n", b">ab"):
        blob, pos, rank = _header_table(text)
        name = text[1:].split()[0].decode()
        dest, off, kept = _lib.fasta_plan(blob, pos, rank, len(text), [name])
        assert dest.tolist() == [0] and kept == 1


class _FakeEngine(object):
    def __init__(self):
        self.set, self.loaded = [], []

    def set_genome(self, off, codes):
        self.set.append((off, codes))

    def load_genome_fasta(self, path, references):
        self.loaded.append(path)
        return np.zeros(len(references) + 1, np.int64), {"kind": "plain"}


def test_load_genome_routes(tmp_path, monkeypatch):
    text = F.record(b"a", F.bases(3, 100)) + F.record(b"b", F.bases(4, 50).lower())
    path = F.write(tmp_path / "r.fa", text, "plain")
    refs = ["b", "a"]
    exp_off, exp_codes = convert.genome_arrays(path, refs)
    monkeypatch.delenv("SVX_GENOME_HOST", raising=False)
    # no engine: the arrays themselves
    off, codes, st = convert.load_genome(None, path, refs)
    assert np.array_equal(off, exp_off) and np.array_equal(codes, exp_codes) and st["route"] == "host"
    # a dict never goes to the device loader
    e = _FakeEngine()
    off, st = convert.load_genome(e, {"a": "ACGT", "b": "gg"}, refs)
    assert off.tolist() == [0, 2, 6] and not e.loaded and e.set[0][1].tolist() == [4, 4, 1, 2, 4, 8] and st["route"] == "host"
    # a path does
    e = _FakeEngine()
    off, st = convert.load_genome(e, path, refs)
    assert e.loaded == [path] and not e.set and st["route"] == "device"
    # the one switch, read at call time
    monkeypatch.setenv("SVX_GENOME_HOST", "1")
    e = _FakeEngine()
    off, st = convert.load_genome(e, path, refs)
    assert not e.loaded and np.array_equal(off, exp_off) and np.array_equal(e.set[0][1], exp_codes) and st["route"] == "host"
    monkeypatch.delenv("SVX_GENOME_HOST")
    # genome_arrays opens by the NAME: a gzip file without ".gz" (and the other way round) is the host parser's to answer
    e = _FakeEngine()
    gz = tmp_path / "named_plain.fa"
    gz.write_bytes(gzip.compress(text))
    convert.load_genome(e, str(gz), refs)
    assert not e.loaded and len(e.set) == 1

    # a loader that hands the file back: the host route loads it
    class Back(_FakeEngine):
        def load_genome_fasta(self, path, references):
            raise _lib.FastaHostRoute("blanks", _abi.SVX_E_FASTA_HOST, {"host_reason": "blanks"})
    e = Back()
    off, st = convert.load_genome(e, path, refs)
    assert np.array_equal(off, exp_off) and st["route"] == "host" and st["device_loader"] == {"host_reason": "blanks"}
