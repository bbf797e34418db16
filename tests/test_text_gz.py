"""BGZF output (svx_text_gz): the DEFLATE encoder of svim_amd/csrc/deflate_core.hpp built for the host (svx_text_gz_host; the kernels write the same bytes for
the same text, tests/test_gpu_text_gz.py holds them to that) judged by zlib, by the host builds of the project's two decoders, under the sanitizers, and
measured against zlib level 1."""
import gzip
import os
import subprocess

import pytest

import text_gz_cases as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "svim_amd", "csrc")


def _inputs():
    vcf, bed = TC.vcf_golden_text(), TC.bed_golden_text()
    return [("vcf_golden", vcf), ("bed_golden", bed), ("vcf_golden_one_block", vcf[:50000]), ("bed_golden_one_block", bed[:50000]),
            ("vcf_golden_tiled", TC.tiled(vcf, 3 * len(vcf) + 17)), ("bed_golden_tiled", TC.tiled(bed, 2 * len(bed) + 5))] + TC.corner_inputs()


def test_round_trip_under_zlib_block_by_block():
    from svim_amd import _lib
    kinds, sizes = {}, {}
    for name, text in _inputs():
        stream = _lib.text_gz_host(text)
        assert gzip.decompress(stream) == text, name
        blocks = TC.walk(stream, text)
        assert len(blocks) == (len(text) + TC.BLOCK - 1) // TC.BLOCK + 1, name
        assert _lib.text_gz_host(text) == stream, name                     # run after run the same bytes
        kinds[name], sizes[name] = [b[3] for b in blocks], len(stream)
    assert _lib.text_gz_host(b"") == TC.EOF_BLOCK
    assert set(kinds["random"][:-1]) == {"stored"} and sizes["random"] == 150000 + 3 * 31 + 28
    assert set(kinds["one_byte"][:-1]) == set(kinds["one_line"][:-1]) == {"dynamic"} and sizes["one_byte"] < 600 and sizes["one_line"] < 3000
    assert kinds["last_block_1"] == ["dynamic", "stored", "eof"] and kinds["last_block_2"] == ["dynamic", "stored", "eof"]
    assert kinds["bases"][:-1] == ["dynamic", "dynamic"] and sizes["bases"] < 70000 * 0.35        # literals only: 2 bits of entropy per byte, coded in < 2.8
    # the repeat exactly 32 768 bytes back is taken (one or two match tokens instead of 300 literals of 6 bits of entropy each); one byte farther it is out of reach
    assert kinds["repeat_at_32768"] == kinds["repeat_at_32769"] == ["dynamic", "eof"] and sizes["repeat_at_32768"] + 150 < sizes["repeat_at_32769"]
    assert all("stored" not in kinds[k] for k in kinds if k.startswith("vcf_golden") or k.startswith("bed_golden"))


def test_the_projects_decoders_read_it(tmp_path):
    """the stream as a BGZF file through the host builds of both decoders (unchanged tools: each compares every block with zlib)"""
    from svim_amd import _lib
    text = TC.tiled(TC.vcf_golden_text(), 200000) + TC.tiled(TC.bed_golden_text(), 200000) + b"".join(t for n, t in TC.corner_inputs() if n in ("bases", "one_byte", "run_258", "run_259"))
    path = str(tmp_path / "t.vcf.gz")
    with open(path, "wb") as fh:
        fh.write(_lib.text_gz_host(text))
    n_blocks = (len(text) + TC.BLOCK - 1) // TC.BLOCK + 1
    core = str(tmp_path / "inflate_host_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DINF_HOST", "-I", CSRC, os.path.join(REPO, "tools", "inflate_host_test.cpp"), "-lz", "-o", core])
    out = subprocess.run([core, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout and "%d BGZF blocks" % n_blocks in out.stdout, (out.stdout[-600:], out.stderr[-2000:])
    lanes = str(tmp_path / "inflate_lanes_host_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(REPO, "tools", "inflate_lanes_host_test.cpp"), "-lz", "-o", lanes])
    out = subprocess.run([lanes, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "%d blocks, 0 mismatches, " % n_blocks in out.stdout, (out.stdout[-600:], out.stderr[-2000:])


def test_encoder_under_the_sanitizers(tmp_path):
    """tools/text_gz_host_test.cpp (the header with -DDEF_HOST) under AddressSanitizer + UndefinedBehaviorSanitizer over a seeded fuzz of the kinds of text above:
    every stream inflates back under zlib, no report (the LDS scratch members are plain arrays here: their bounds are checked); and over the phase-level cases
    of tests/deflate_encode_cases.py (`cases FILE`): every block equals the model's, with the staging window of the 64 x 48-bit batches, every token buffer
    and every slot a heap block of its own size"""
    out = str(tmp_path / "text_gz_host_asan")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DDEF_HOST", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I", CSRC, os.path.join(REPO, "tools", "text_gz_host_test.cpp"), "-lz", "-o", out], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("no sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([out, "fuzz", "7", "3000"], capture_output=True, text=True, timeout=1200)
    assert run.returncode == 0 and "3000 buffers, 0 mismatches" in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    stored, dynamic = (int(run.stdout.split(w)[0].split()[-1]) for w in (" stored", " dynamic"))
    assert stored > 300 and dynamic > 1000, run.stdout[-300:]
    import deflate_encode_cases as DC
    cases = str(tmp_path / "cases.bin")
    n_blocks = DC.write_case_file(cases)
    assert sum(1 for c in DC.bits_cases() if c["name"].startswith("items_64x48_at_")) == 32
    run = subprocess.run([out, "cases", cases], capture_output=True, text=True, timeout=1200)
    assert run.returncode == 0 and "cases: %d blocks, 0 mismatches" % n_blocks in run.stdout, (run.stdout[-500:], run.stderr[-3000:])


def test_size_against_zlib_level_1():
    """ours <= 1.20 x (zlib level 1 on the same 65 280-byte blocks, framed as BGZF) on the reference's own VCF lines, its BED lines, and a seeded VCF text with
    SEQS / READS / ZMWS; no block of them stored, every block smaller than its text.  Measured (the encoder is deterministic: one run is the measurement):
    ours / zlib1 = 0.951 (VCF golden), 0.904 (BED golden), 0.957 (seeded); ours / text = 0.128, 0.029, 0.345."""
    from svim_amd import _lib
    for name, text in (("vcf_golden", TC.vcf_golden_text()), ("bed_golden", TC.bed_golden_text()), ("seeded_vcf", TC.seeded_vcf_text())):
        assert len(text) > 3 * TC.BLOCK, name
        stream = _lib.text_gz_host(text)
        yard = TC.zlib1_bgzf_size(text)
        print("%s: %d bytes of text, ours %d, zlib level 1 %d, ours / zlib1 = %.4f, ours / text = %.4f" % (name, len(text), len(stream), yard, len(stream) / yard, len(stream) / len(text)))
        blocks = TC.walk(stream, text)
        ends = [b[0] for b in blocks[1:]] + [len(stream)]
        for (at, _, isize, kind), end in zip(blocks[:-1], ends):
            assert kind == "dynamic" and end - at < isize, (name, at, kind, end - at, isize)
        assert len(stream) <= 1.20 * yard, (name, len(stream), yard)
    assert len(TC.seeded_vcf_text()) > 2_000_000
