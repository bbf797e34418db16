"""Shared by tests/test_text_gz.py and tests/test_gpu_text_gz.py: the input texts of the BGZF writer (svx_text_gz), a BGZF block walker that checks every
field against zlib, and the size yardstick (zlib level 1 on the same 65 280-byte blocks, framed as BGZF)."""
import gzip
import json
import os
import struct
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _strings(x, out):
    if isinstance(x, str):
        if len(x) > 40:
            out.append(x)
    elif isinstance(x, dict):
        for v in x.values():
            _strings(v, out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _strings(v, out)
    return out


def golden_text(name):
    """every string of a golden file longer than 40 characters, joined by newlines: the reference's own lines"""
    with gzip.open(os.path.join(HERE, "golden", name), "rt") as fh:
        return ("\n".join(_strings(json.load(fh), [])) + "\n").encode("utf-8")


def vcf_golden_text():
    return golden_text("g_vcf_cases.json.gz")


def bed_golden_text():
    return golden_text("g_bed_cases.json.gz")


def tiled(text, n):
    return (text * (n // max(1, len(text)) + 1))[:n]


def seeded_vcf_text(n_candidates=6000, seed=5):
    """variants.vcf lines with SEQS, READS and ZMWS over hand-built candidates: random inserted sequences of 40 .. 300 bases, PacBio-style read names (the
    workload of tools/vcf_rate.py in small; no GPU: SVIM_COMBINE.vcf_body_python makes the lines)"""
    import vcf_cases as VC
    from svim_amd import SVIM_COMBINE, candidates as K
    rng = np.random.default_rng(seed)
    n_reads = 4 * n_candidates
    names = ["m64011_190830_220126/%d/%d_%d" % (4000 + 3 * (k // 2), 100 * k, 100 * k + 9000) for k in range(n_reads)]
    contigs = ["chr%d" % (k + 1) for k in range(8)]

    def members():
        k = int(rng.integers(2, 12))
        return [VC.Sig(names[int(r)], "".join("ACGT"[b] for b in rng.integers(0, 4, int(rng.integers(40, 301))))) for r in rng.integers(0, n_reads, k)]

    ins, dele, inv, bnd = [], [], [], []
    for k in range(n_candidates):
        c, pos = contigs[int(rng.integers(0, 8))], int(rng.integers(1000, 5_000_000))
        score, sd1, sd2 = int(rng.integers(1, 60)), float(rng.integers(0, 4000)) / 100.0, float(rng.integers(0, 4000)) / 100.0
        kind = k % 8
        if kind < 5:
            ins.append(K.CandidateNovelInsertion(c, pos, pos + int(rng.integers(40, 301)), "", members(), score, sd1, sd2))
        elif kind < 7:
            dele.append(K.CandidateDeletion(c, pos, pos + int(rng.integers(40, 5000)), members(), score, sd1, sd2))
        else:
            inv.append(K.CandidateInversion(c, pos, pos + int(rng.integers(100, 9000)), members(), score, sd1, sd2))
    o = types.SimpleNamespace(symbolic_alleles=True, insertion_sequences=True, read_names=True, zmws=True, tandem_duplications_as_insertions=False,
                              interspersed_duplications_as_insertions=False)
    lines = SVIM_COMBINE.vcf_body_python([], inv, [], dele, ins, bnd, list(VC.ALL_TYPES), o, False, None)
    return "".join(l + "\n" for l in lines).encode("utf-8")


def zlib1_bgzf_size(text):
    """what `bgzip -l 1` writes for text: zlib level 1 raw DEFLATE of every 65 280-byte block + 26 bytes of frame each, + the end-of-file block"""
    total = 28
    for at in range(0, len(text), BLOCK):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(c.compress(text[at:at + BLOCK]) + c.flush()) + 26
    return total


def walk(stream, text):
    """every BGZF block of `stream` (one file: data blocks, then the end-of-file block) against the slice of `text` it holds -> list of (compressed offset,
    text offset, text bytes, kind) with kind 'stored' / 'dynamic' / 'eof'; asserts every field"""
    assert stream[-28:] == EOF_BLOCK, "the stream does not end with the BGZF end-of-file block"
    blocks, at, uat = [], 0, 0
    while at < len(stream):
        size = _header(stream, at) + 1
        assert at + size <= len(stream), "BSIZE runs past the stream"
        payload = stream[at + 18:at + size - 8]
        crc, isize = struct.unpack_from("<II", stream, at + size - 8)
        last = at + size == len(stream)
        if last:
            assert stream[at:at + size] == EOF_BLOCK and isize == 0
            kind = "eof"
        else:
            piece = text[uat:uat + isize]
            assert len(piece) == isize and isize > 0
            assert isize == BLOCK or uat + isize == len(text), "a data block other than the last holds %d bytes" % isize
            assert crc == zlib.crc32(piece), "CRC32 of block at %d" % at
            assert zlib.decompress(payload, -15) == piece, "payload of block at %d" % at
            btype = (payload[0] >> 1) & 3
            assert payload[0] & 1 == 1 and btype in (0, 2), "one final block, stored or dynamic"
            kind = "stored" if btype == 0 else "dynamic"
        blocks.append((at, uat, isize, kind))
        at += size
        uat += isize
    assert uat == len(text) and at == len(stream)
    return blocks


def _header(stream, at):
    id1, id2, cm, flg, mtime, xfl, os_, xlen, si1, si2, slen, bsize = struct.unpack_from("<BBBBIBBHBBHH", stream, at)
    assert (id1, id2, cm, flg, mtime, xfl, os_, xlen, si1, si2, slen) == (31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2), "BGZF header at %d" % at
    return bsize


def corner_inputs():
    """(name, bytes): the corners of the format and of the match finder"""
    rng = np.random.default_rng(17)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()      # noqa: E731
    line = b"chr7\t1204\t1560\tsvim.DEL.12;0.91;3\t17\tm64011_190830_220126/4012/300_9300,m64011_190830_220126/4015/500_9500\n"
    out = [("random", rnd(150000)), ("one_byte", b"A" * 140000), ("one_line", tiled(line, 200000))]
    for n in (0, 1, 2, 3, 65279, 65280, 65281, 130560, 130561):
        out.append(("len_%d" % n, tiled(line, n)))
    out.append(("last_block_1", tiled(line, BLOCK) + b"x"))
    out.append(("last_block_2", tiled(line, BLOCK) + b"xy"))
    # 300 bytes of a 64-letter alphabet (no repeat inside), one letter repeated up to the distance, the 300 bytes again: their only earlier occurrence lies
    # exactly d back, and the run between the two leaves their entries of the hash table alone
    piece = bytes(48 + int(k) for k in rng.integers(0, 64, 300))
    for d in (32768, 32769):
        out.append(("repeat_at_%d" % d, piece + b"~" * (d - 300) + piece + b"~" * 40))
    for run in (258, 259):
        out.append(("run_%d" % run, rnd(50) + b"G" * (run + 1) + rnd(50) + b"T" * (run + 1) + rnd(7)))
    out.append(("bases", bytes(b"ACGT"[k] for k in rng.integers(0, 4, 70000))))
    return out
