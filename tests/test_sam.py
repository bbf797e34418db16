"""SAM text -> BAM records on the CPU: the host build (svx_sam_convert_host, svx_sam_header_host: csrc/sam_host.cpp over csrc/sam_core.hpp) equals the definition
(svim_amd/sam.py) byte for byte on every corner line of tests/sam_cases.py and on two seeded files; the definition itself is held to the project's independent
SAM and BAM readers (records.AlignmentFile), the integer widths to the stated rule; COLLECT sees the same records either way; every refusal gives its status
and its line; too little room reports the size; the sanitizer fuzz of the host core ends clean.  tests/test_gpu_sam.py holds the device build to the same."""
import os
import struct
import subprocess

import pytest

import bam_sort_cases as SC
import helpers as H
import sam_cases as SAMC
from svim_amd import _abi, _lib, batch, records, sam

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def cases():
    ls = SAMC.lines()
    return ls, [sam.record_bytes(l, SAMC.TID) for _, l in ls]


def test_host_build_equals_definition_on_every_case(cases):
    ls, want = cases
    for (name, l), w in zip(ls, want):
        got, n = _lib.sam_convert_host(l, SAMC.REFS)
        assert n == 1 and got == w, name
    for last_newline in (True, False):
        got, n = _lib.sam_convert_host(SAMC.text(ls, last_newline), SAMC.REFS)
        assert n == len(ls) and got == b"".join(want), last_newline
    assert _lib.sam_header_host(SAMC.HEADER) == sam.header_bytes(SAMC.HEADER)
    assert _lib.sam_header_host(b"") == sam.header_bytes(b"") == b"BAM\1" + bytes(8)


@pytest.mark.parametrize("seed", [11, 12])
def test_host_build_equals_definition_on_a_seeded_file(seed):
    text, ls = SAMC.seeded_file(seed, 20000)
    header, want = sam.convert(text)
    got, n = _lib.sam_convert_host(text, SAMC.REFS)
    assert n == 20000 and got == b"".join(want)
    assert header == _lib.sam_header_host(SAMC.HEADER)


def test_long_cigar_and_bin_rules(cases):
    ls, want = cases
    by = {name: w for (name, _), w in zip(ls, want)}

    def fixed(w):
        return struct.unpack_from("<iiBBHHHiiii", w, 4)
    f = fixed(by["cigar65535"])
    assert f[5] == 65535 and b"CGBI" not in by["cigar65535"]
    w = by["cigar65536"]
    f = fixed(w)
    l_name = f[2]
    assert f[5] == 2 and struct.unpack_from("<2I", w, 36 + l_name) == ((51 << 4) | 4, (3 * 32768 << 4) | 3)          # 51S, then the 32768 x (2M + 1D) reference bases as N
    tail = w[-(8 + 4 * 65536):]
    assert tail[:4] == b"CGBI" and struct.unpack_from("<I", tail, 4)[0] == 65536 and struct.unpack_from("<2I", tail, 8) == ((2 << 4) | 0, (1 << 4) | 2)
    assert fixed(by["rname_star"])[:2] == (-1, -1) and fixed(by["rname_star"])[4] == 4680
    assert fixed(by["unmapped_with_position_zero"])[:2] == (1, -1) and fixed(by["unmapped_with_position_zero"])[4] == 4680
    assert fixed(by["cigar_without_reference_bases"])[4] == sam.reg2bin(4241, 4242)
    assert fixed(by["rnext_equal"])[8] == 1 and fixed(by["rnext_name_tlen_min"])[8:] == (2, 2 ** 31 - 2, -2 ** 31)


def test_integer_tags_take_the_smallest_type(cases):
    ls, want = cases
    types_ = {-2 ** 31: b"i", -32769: b"i", -32768: b"s", -129: b"s", -128: b"c", -1: b"c", 0: b"C", 255: b"C", 256: b"S", 65535: b"S", 65536: b"I", 2 ** 32 - 1: b"I"}
    width = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4}
    for (name, _), w in zip(ls, want):
        if not name.startswith("int"):
            continue
        v = int(name[3:])
        aux = w[4 + 32 + 2 + 4 + 2 + 3:]
        t = aux[2:3]
        assert aux[:2] == b"XI" and t == types_[v], name
        assert int.from_bytes(aux[3:3 + width[t]], "little", signed=t.islower()) == v, name
        assert aux[3 + width[t]:][:2] == b"XJ" and len(aux) == 2 * (3 + width[t]), name


def _norm_tags(tags):
    out = {}
    for k, v in tags.items():
        if isinstance(v, float):
            v = ("f", struct.pack("<f", v) if v == v else b"nan")
        out[k] = v
    return out


def _sam_side_tags(l):
    """the tags of a line as the BAM reader shows them: B arrays as lists, floats through float32"""
    out = {}
    for fld in l.decode("latin-1").split("\t")[11:]:
        k, t, v = fld.split(":", 2)
        if k in out:
            continue
        if t == "i":
            out[k] = int(v)
        elif t == "f":
            x = struct.unpack("<f", sam._float(v.encode()))[0]
            out[k] = ("f", struct.pack("<f", x) if x == x else b"nan")
        elif t == "B":
            items = v.split(",")[1:]
            out[k] = [struct.unpack("<f", sam._float(i.encode()))[0] for i in items] if v[0] == "f" else [int(i) for i in items]
        else:
            out[k] = v
    return out


def test_definition_read_back_by_the_projects_readers(cases, tmp_path):
    """an independent check of the definition: records.AlignmentFile reads the BAM made of the definition's bytes and the SAM text it was made from"""
    ls, want = cases
    path = str(tmp_path / "cases.bam")
    SC.write_raw(path, sam.header_bytes(SAMC.HEADER), want)
    from_bam = list(records.AlignmentFile(path).fetch())
    from_sam = list(records.AlignmentFile(text=SAMC.text(ls).decode("latin-1")).fetch())
    assert len(from_bam) == len(from_sam) == len(ls)
    nt = set(sam.NT16)
    for (name, l), a, b in zip(ls, from_bam, from_sam):
        assert (a.query_name, a.flag, a.reference_id, a.reference_start, a.mapping_quality, a.next_reference_id, a.next_reference_start, a.template_length) == \
               (b.query_name, b.flag, b.reference_id, b.reference_start, b.mapping_quality, b.next_reference_id, b.next_reference_start, b.template_length), name
        assert (a.cigartuples or []) == (b.cigartuples or []), name
        seq = l.split(b"\t")[9].decode("latin-1")
        assert (a.query_sequence or "") == ("" if seq == "*" else "".join(c.upper() if c.upper() in nt else "N" for c in seq)), name
        got = _norm_tags(a._tags)
        exp = _sam_side_tags(l)
        if got != exp:
            for k in exp:                                   # (nan != nan inside a list)
                assert repr(got.get(k)) == repr(exp[k]), (name, k)
            assert set(got) == set(exp), name
    # qualities are not on the readers' path: against the text directly
    for (name, l), w in zip(ls, want):
        f = l.split(b"\t")
        l_seq = 0 if f[9] == b"*" else len(f[9])
        l_name, n_cig = w[12], struct.unpack_from("<H", w, 16)[0]
        q = w[36 + l_name + 4 * n_cig + (l_seq + 1) // 2:][:l_seq]
        assert q == (b"\xff" * l_seq if f[10] == b"*" else bytes(c - 33 for c in f[10])), name


def test_collect_on_the_converted_golden_equals_the_text_route(tmp_path, oracle):
    """tests/golden/chimeric_read.sam converted by the definition and by the host build; COLLECT (the oracle's, on the CPU) over the BAM equals COLLECT over the text"""
    src = os.path.join(HERE, "golden", "chimeric_read.sam")
    text = open(src, "rb").read()
    header, recs = sam.convert(text)
    host, n = _lib.sam_convert_host(text, [n for n, _ in sam.dictionary(sam.split_text(text)[0])])
    assert n == len(recs) and host == b"".join(recs) and _lib.sam_header_host(sam.split_text(text)[0]) == header
    path = str(tmp_path / "chimeric.bam")
    SC.write_raw(path, header, recs)
    o = H.options({"min_mapq": 20, "min_sv_size": 40, "max_sv_size": 100000, "segment_gap_tolerance": 10, "segment_overlap_tolerance": 5, "all_bnds": True})
    p = _abi.Params.from_options(o)
    a, b = records.AlignmentFile(path), records.AlignmentFile(src)
    assert a.references == b.references and a.lengths == b.lengths and a.header.get("HD") == b.header.get("HD")
    mode = "queryname" if a.header.get("HD", {}).get("SO") == "queryname" else "coordinate"
    sig_a, bnd_a = oracle.collect(batch.build_batch(a, o, mode=mode), p)
    sig_b, bnd_b = oracle.collect(batch.build_batch(b, o, mode=mode), p)
    assert sig_b.n > 0 and sig_a.first_difference(sig_b) is None and bnd_a.first_difference(bnd_b) is None


def test_line_of_record_is_the_inverse(cases):
    """sam.line_of_record (tools write SAM text of BAM records with it): the line of a record converts back to the same record"""
    ls, want = cases
    for (name, _), w in zip(ls, want):
        assert sam.record_bytes(sam.line_of_record(w, SAMC.REFS), SAMC.TID) == w, name


def test_every_refusal_returns_its_status_and_line(cases):
    ls, _ = cases
    good = [l for name, l in ls if name in ("no_aux", "rnext_equal", "seq17_qual")]
    for name, bad, code in SAMC.refusals():
        with pytest.raises(sam.SamError) as d:
            sam.record_bytes(bad, SAMC.TID)
        assert d.value.code == code, name
        text = SAMC.HEADER + b"\n".join(good + [bad] + good) + b"\n"
        want_line = SAMC.HEADER.count(b"\n") + len(good) + 1
        with pytest.raises(sam.SamError) as h:
            _lib.sam_convert_host(text, SAMC.REFS)
        assert (h.value.code, h.value.line) == (code, want_line), (name, str(h.value))
        with pytest.raises(sam.SamError) as d2:
            sam.convert(text)
        assert (d2.value.code, d2.value.line) == (code, want_line), name
    with pytest.raises(sam.SamError):
        sam.header_bytes(b"@HD\tVN:1.6\n", have_alignments=True)
    with pytest.raises(sam.SamError):
        sam.convert(b"@HD\tVN:1.6\n" + good[0] + b"\n")


def test_several_faults_report_the_first_in_the_stated_order():
    n_head = SAMC.HEADER.count(b"\n")
    for name, ls, k, code in SAMC.several_faults():
        text = SAMC.HEADER + b"\n".join(ls) + b"\n"
        for convert in (lambda t: _lib.sam_convert_host(t, SAMC.REFS), sam.convert):
            with pytest.raises(sam.SamError) as e:
                convert(text)
            assert (e.value.code, e.value.line) == (code, n_head + k + 1), (name, str(e.value))


def test_float_grammar_and_fast_path_bounds():
    """what the float grammar takes is what both float() and strtod take; a literal with more fractional digits than the fast path counts is left to strtod,
    in the builds and by the definition's own rule, and converts to the same bytes"""
    for t in ("1.", ".5", "+.5e3", "INF", "-Infinity", "1e400", "-1e400"):
        ln = SAMC.line(aux=["XX:f:" + t], **SAMC.GOOD)
        assert _lib.sam_convert_host(SAMC.HEADER + ln + b"\n", SAMC.REFS)[0] == sam.record_bytes(ln, SAMC.TID), t
    assert sam.record_bytes(SAMC.line(aux=["XX:f:1e400"], **SAMC.GOOD), SAMC.TID)[-4:] == struct.pack("<f", float("inf"))
    for frac, fast in ((400, True), (401, False)):
        t = "0." + "0" * (frac - 1) + "5e%d" % frac                          # one significant digit behind frac - 1 zeros, times 10^frac: 5
        assert sam.float_fast_path(t.encode()) is fast
        ln = SAMC.line(aux=["XX:f:" + t], **SAMC.GOOD)
        rec = _lib.sam_convert_host(SAMC.HEADER + ln + b"\n", SAMC.REFS)[0]
        assert rec == sam.record_bytes(ln, SAMC.TID) and rec[-4:] == struct.pack("<f", float(t)), frac
    # the far-fetched one: 100 001 fractional digits and the exponent that undoes them
    t = "0." + "0" * 100000 + "5e100001"
    ln = SAMC.line(aux=["XX:f:" + t], **SAMC.GOOD)
    assert _lib.sam_convert_host(SAMC.HEADER + ln + b"\n", SAMC.REFS)[0][-4:] == struct.pack("<f", float(t)) and not sam.float_fast_path(t.encode())


def test_file_order_route_and_what_is_sam_text(tmp_path):
    """sam_to_bam(sort=False) is the host's route: header and records of the definition in file order, through the encoder; and what NativeBam takes for SAM text"""
    import gzip
    from svim_amd import harness
    from svim_amd.bamio import is_sam_text, NativeBam
    text, ls = SAMC.seeded_file(5, 300)
    header, recs = sam.convert(text)
    src, out = str(tmp_path / "a.sam"), str(tmp_path / "a.bam")
    with open(src, "wb") as fh:
        fh.write(text)
    st = harness.sam_to_bam(src, out, sort=False, index=False)
    assert gzip.open(out, "rb").read() == header + b"".join(recs) and st["n_records"] == 300 and not os.path.exists(out + ".bai")
    assert open(out, "rb").read() == _lib.text_gz_host(header + b"".join(recs))
    with pytest.raises(ValueError):
        harness.sam_to_bam(src, out, sort=False, index=True)
    with pytest.raises(ValueError):
        harness.sam_to_bam(out, str(tmp_path / "b.bam"), sort=False, index=False)
    assert is_sam_text(src) and not is_sam_text(out) and not is_sam_text(str(tmp_path / "missing.bam"))
    junk, empty, headerless = str(tmp_path / "junk.bam"), str(tmp_path / "empty.bam"), str(tmp_path / "noheader.sam")
    for path, data in ((junk, b"\x00\x01\x02 not BGZF"), (empty, b""), (headerless, ls[0] + b"\n")):
        with open(path, "wb") as fh:
            fh.write(data)
    assert not is_sam_text(junk) and not is_sam_text(empty) and is_sam_text(headerless)
    # paths that are no SAM text fail as they did: in svx_bam_open, with its message
    for path in (junk, str(tmp_path / "missing.bam")):
        with pytest.raises(_lib.SvxError) as e:
            NativeBam(path)
        assert "svx_bam_open" in str(e.value), str(e.value)


def test_too_little_room_reports_the_size(cases):
    ls, want = cases
    text, total = SAMC.text(ls), sum(len(w) for w in want)
    for cap in (0, 1, len(want[0]), total - 1):
        with pytest.raises(_lib.SvxError) as e:
            _lib.sam_convert_host(text, SAMC.REFS, cap=cap)
        assert e.value.code == _abi.SVX_E_CAPACITY and e.value.needed == total, cap
    assert _lib.sam_convert_host(text, SAMC.REFS, cap=total)[0] == b"".join(want)


def test_sanitizer_fuzz_of_the_host_core_ends_clean(tmp_path):
    """tools/sam_host_test.cpp: the host core over mutated, truncated and overlong lines under AddressSanitizer and UBSan - a stand-alone program, no GPU"""
    exe = str(tmp_path / "sam_host_test")
    src = [os.path.join(REPO, "tools", "sam_host_test.cpp"), os.path.join(REPO, "svim_amd", "csrc", "sam_host.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    # asked BEFORE the build: a toolchain without the sanitizer runtime cannot link the smallest program; a failure of the real build is then a failure
    if subprocess.run(["g++", *san, probe, "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime in this toolchain")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *san, "-fno-omit-frame-pointer", "-I", os.path.join(REPO, "svim_amd", "csrc"), "-o", exe] + src,
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([exe, "7", "4000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode("utf-8", "replace")[-4000:]
    assert b"sam_host_test ok" in r.stdout
