"""The DEFLATE decoders ON THE GPU (svim_amd/csrc/bgzf.hip: one wave per block, and SVX_INFLATE_LANES=1: one lane per block with the wave decoder behind it) on the
streams of tests/deflate_streams.py - what zlib's compressor never writes, and every rule of the format broken once -, and through the products that inflate on
the device: the device-resident BAM reader, the reader with GPU inflate, the FASTA genome loader.  Only here do the LDS ring, the read-back of far match sources
from global memory and the fence in front of it exist for real.  tests/test_deflate_streams.py runs the same corpus through the host builds under the sanitizers:
a rule-breaking stream reaches the GPU only from that corpus.  One process, one context."""
import zlib

import numpy as np
import pytest

import deflate_streams as DS
import fasta_cases as F
import foreign_bam as FB
import helpers as H
from svim_amd import _lib, convert, synth

pytestmark = pytest.mark.gpu
DECODERS = ("wave_per_block", "lane_per_block")


def _select(monkeypatch, decoder):
    if decoder == "lane_per_block":
        monkeypatch.setenv("SVX_INFLATE_LANES", "1")
    else:
        monkeypatch.delenv("SVX_INFLATE_LANES", raising=False)


@pytest.fixture(scope="module")
def sound():
    """[(name, stream, payload)]; the reference is zlib's answer, which tests/test_deflate_streams.py holds equal to the intended payload"""
    out = [(c[0], c[2], zlib.decompress(c[2], -15)) for c in DS.corpus() if c[3] != DS.INVALID]
    assert len(out) > 100
    return out


@pytest.mark.parametrize("decoder", DECODERS)
def test_sound_streams_inflate_to_zlibs_bytes(monkeypatch, sound, decoder):
    """all of them in one call, then rotated and cut into calls of 7, 64 and 100 jobs: every stream at several job indices (and, in the lane decoder, in several
    lanes and beside different neighbours)"""
    _select(monkeypatch, decoder)
    f = _lib.Inflater(0)
    try:
        got = f.inflate([(s, len(p)) for _, s, p in sound]).tobytes()
        at = 0
        for name, _, p in sound:
            assert got[at:at + len(p)] == p, (decoder, name)
            at += len(p)
        assert at == len(got)
        for rot, per_call in ((1, 7), (13, 64), (29, 100)):
            order = sound[rot:] + sound[:rot]
            for lo in range(0, len(order), per_call):
                part = order[lo:lo + per_call]
                got = f.inflate([(s, len(p)) for _, s, p in part]).tobytes()
                at = 0
                for name, _, p in part:
                    assert got[at:at + len(p)] == p, (decoder, name, rot, per_call)
                    at += len(p)
    finally:
        f.close()


@pytest.mark.parametrize("decoder", DECODERS)
def test_rule_breaking_streams_are_reported_and_the_inflater_goes_on(monkeypatch, sound, decoder):
    """one rule-breaking stream per call among sound neighbours: the call raises, and the same Inflater then decodes the sound blocks.  Error REPORTING on bounded,
    well-formed buffers - each of these streams went through the sanitizer builds of both decoders first (tests/test_deflate_streams.py)."""
    _select(monkeypatch, decoder)
    near = [(s, len(p)) for _, s, p in sound if 0 < len(p) < 6000][:8]
    want = b"".join(zlib.decompress(s, -15) for s, _ in near)
    bad = [(c[0], c[2], c[4]) for c in DS.corpus() if c[3] == DS.INVALID]
    assert len(bad) > 50 and len(near) == 8
    f = _lib.Inflater(0)
    try:
        accepted = []
        for k, (name, stream, size) in enumerate(bad):
            cut = k % 7
            try:
                f.inflate(near[:cut] + [(stream, size)] + near[cut:])
                accepted.append(name)
            except Exception:
                pass
            assert f.inflate(near).tobytes() == want, (decoder, "after", name)
        assert not accepted, (decoder, accepted)
    finally:
        f.close()


def _records():
    contigs = [("chr1", 150000), ("chr2", 60000)]
    refs = synth.make_reference(3, contigs)
    names, lens = [c[0] for c in contigs], [c[1] for c in contigs]
    recs = synth.coordinate_sort(synth.planted_reads(5, 150, refs, names, lens, n_sites=12, types=("DEL", "INS", "INV")))
    import random
    rng = random.Random(9)
    rb = [FB.record_bytes(a, FB.decorate(rng, a, k), bytes(rng.randrange(2, 45) for _ in range(len(a._seq or ""))) if k % 2 else None) for k, a in enumerate(recs)]
    return names, lens, recs, rb


def test_bam_of_constructed_blocks_through_the_device_readers(tmp_path, monkeypatch):
    """a BAM whose BGZF blocks come from the three encoder policies in turn (tests/foreign_bam.py, deflate=): the device-resident reader - whole file in one chunk,
    one block per chunk, three - and the reader with GPU inflate deliver every array of every batch as the host reader does, with either decoder"""
    from svim_amd.bamio import NativeBam
    names, lens, recs, rb = _records()
    path = str(tmp_path / "constructed.bam")
    order = [DS.policy_one_block, DS.policy_short_blocks, DS.policy_static]
    n_blocks = FB.write(path, names, lens, rb, layout="htslib", deflate=order, block_payload=24000, tids=[a.reference_id for a in recs])
    assert n_blocks >= 6

    def read_all(setup, stats=None):
        nb = NativeBam(path, threads=2)
        setup(nb)
        out = []
        while True:
            b, n = nb.read_batch(61, 20, "coordinate")
            if n == 0:
                break
            out.append(nb.batch_arrays(b))
        if stats is not None:
            stats.update(nb.gpu_inflate_stats())
        nb.close()
        return out

    monkeypatch.setenv("SVX_BAM_GPU_SUB", "16")                          # (sub-batches of 16 blocks, chunks of 60: the GPU takes its share of this small file)
    monkeypatch.setenv("SVX_BAM_CHUNK_BLOCKS", "60")
    host = read_all(lambda nb: None)
    rows = H.concat_batch_rows(host)
    H.assert_rows_are_the_written_records(rows, recs, "host reader")
    for decoder in DECODERS:
        _select(monkeypatch, decoder)
        st = {}
        both = read_all(lambda nb: nb.set_gpu_inflate(0), st)
        assert len(both) == len(host) and st["gpu_blocks"] > 0, st
        for a, b in zip(host, both):
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(a[k], b[k]), (decoder, "gpu inflate", k)
        for chunk_blocks in (None, "1", "3"):
            if chunk_blocks:
                monkeypatch.setenv("SVX_BAM_DEV_CHUNK_BLOCKS", chunk_blocks)
            else:
                monkeypatch.delenv("SVX_BAM_DEV_CHUNK_BLOCKS", raising=False)
            dev = read_all(lambda nb: nb.set_device_decode(0))
            assert H.concat_batch_rows(dev) == rows, (decoder, "device reader", chunk_blocks)
        monkeypatch.delenv("SVX_BAM_DEV_CHUNK_BLOCKS", raising=False)


def test_fasta_of_constructed_blocks_through_the_genome_loader(tmp_path, monkeypatch):
    """a bgzip-style FASTA whose blocks come from the encoder policies: convert.load_genome takes the device route and loads what genome_arrays reads"""
    refs = synth.make_reference(7, [("chrA", 90000), ("chrB", 30011)])
    text = "".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in refs.items()).encode("ascii")
    order = [DS.policy_one_block, DS.policy_static, DS.policy_short_blocks]
    blocks = [FB.bgzf_block(text[i:i + 30000], encoder=order[(i // 30000) % 3]) for i in range(0, len(text), 30000)]
    path = str(tmp_path / "constructed.fa.gz")
    with open(path, "wb") as fh:
        fh.write(b"".join(blocks) + FB.EOF_BLOCK)
    exp_off, exp_codes = convert.genome_arrays(path, list(refs))
    eng = _lib.Engine(0)
    try:
        for decoder in DECODERS:
            _select(monkeypatch, decoder)
            eng.set_genome(np.zeros(1, np.int64), np.full(1, 9, np.uint8))
            off, st = convert.load_genome(eng, path, list(refs))
            assert st["route"] == "device" and "device_loader" not in st and st["kind"] == "bgzf", st
            got_off, got_codes = eng.fetch_genome()
            assert np.array_equal(off, exp_off) and np.array_equal(got_off, exp_off) and np.array_equal(got_codes, exp_codes), decoder
    finally:
        eng.close()
