"""Corner lines for SAM text -> BAM records (svim_amd/sam.py, csrc/sam_host.cpp, csrc/sam.hip): seeded alignment lines and their header, the smallest shapes at
which the kernels can go wrong.  tests/test_sam.py holds the definition and the host build to them on the CPU, tests/test_gpu_sam.py the device build on the GPU.

    SEQ / QUAL  lengths 0 ("*"), 1, 2, 15, 16, 17, 63, 64, 65 and 4097, each with qualities and with "*"; IUPAC and lower-case bases, bytes outside the alphabet
    QNAME       lengths 1 to 17 and 254: every source and destination misalignment mod 16 of what follows the name
    CIGAR       "*", 1, 63, 64 and 65 operations (64 text bytes are one step of a wave), lengths of 1 and 9 digits, one record at 65 535 and one at 65 536
                operations (the second holds the placeholder and CG:B:I)
    aux         i at every width edge (-2^31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2^32 - 1); floats on the fast path and off it (17
                digits, 1e-40, inf, nan, a value whose double and float roundings disagree); A, H, an empty Z, an SA:Z of 5 kB, B of every subtype, an empty
                array, a B:f with values off the fast path; no aux at all; more tags than one step holds
    fixed       RNAME "*", RNEXT "=" and a name, an unmapped record with POS 0 (bin 4680), TLEN at both ends of its range
    file        the last line without its newline (text(..., last_newline=False))
    refusals    one line per refusal, with the status the definition gives it

Test infrastructure only."""
import random
from decimal import Decimal, getcontext

REFS = ["chr1", "chr2", "chrM_long_name"]
LENS = [300000000, 48000000, 16569]
HEADER = ("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(REFS, LENS)) + "@PG\tID:aligner\tPN:aligner\n").encode("ascii")
TID = {n: i for i, n in enumerate(REFS)}

getcontext().prec = 80
# 1 + 2^-24 + 2^-55: its nearest double is 1 + 2^-24, the tie between two floats, which goes to 1.0; rounded to float at once it would be 1 + 2^-23
DOUBLE_ROUNDED = str(Decimal(1) + Decimal(2) ** -24 + Decimal(2) ** -55)
FAST_FLOATS = ["1.5", "-0", "0", "3.14159", "1e22", "123456789012345", "0.000001", "1E-5", ".5", "5.", "-2.5e-3", "+7", "1e-22", "16777217", "0.1"]
SLOW_FLOATS = ["0.12345678901234567", "1e-40", "inf", "-inf", "nan", "1e23", "1234567890123456", "3.4e38", "1e39", DOUBLE_ROUNDED]
INTS = [-2 ** 31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2 ** 32 - 1]


def line(qname="r", flag=0, rname="chr1", pos=100, mapq=60, cigar="*", rnext="*", pnext=0, tlen=0, seq="*", qual="*", aux=()):
    return "\t".join([qname, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual] + list(aux)).encode("latin-1")


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _qual(rng, n):
    return "".join(chr(rng.randrange(33, 127)) for _ in range(n))


def _cigar(rng, n_ops, digits=None):
    out = []
    for k in range(n_ops):
        n = rng.randrange(1, 10) if digits is None else (rng.randrange(1, 10) if digits == 1 else rng.randrange(100000000, 2 ** 28))
        out.append("%d%s" % (n, "MIDNSHP=X"[(k * 5 + rng.randrange(2)) % 9]))
    return "".join(out)


def lines():
    """[(name of the case, line)]"""
    rng = random.Random(20240607)
    out = []
    name_len = list(range(1, 18)) + [254]
    k = 0
    for n in (0, 1, 2, 15, 16, 17, 63, 64, 65, 4097):
        for with_qual in (True, False):
            qn = _seq(rng, name_len[k % len(name_len)], "abcdefghijklmnopqrstuvwxyz0123456789_/")
            k += 1
            seq = _seq(rng, n) if n else "*"
            out.append(("seq%d_%s" % (n, "qual" if with_qual else "noqual"),
                        line(qn, flag=16 * (k & 1), pos=1000 * k + 1, cigar="%dM" % n if n else "*", seq=seq, qual=_qual(rng, n) if (with_qual and n) else "*",
                             aux=["NM:i:%d" % k])))
    for ln in name_len:
        out.append(("qname%d" % ln, line(_seq(rng, ln, "ABCXYZabcxyz0189:#"), pos=5000 + ln, cigar="17M", seq=_seq(rng, 17), qual=_qual(rng, 17), aux=["RG:Z:g%d" % ln])))
    out.append(("iupac_lower_and_other", line("iupac", pos=7, cigar="40M", seq="=ACMGRSVTWYHKDBNacmgrsvtwyhkdbn.-xzEFIJ01", qual="*")))
    for n_ops in (1, 63, 64, 65):
        for digits in (1, 9):
            out.append(("cigar%d_digits%d" % (n_ops, digits), line("c%d_%d" % (n_ops, digits), pos=12345, cigar=_cigar(rng, n_ops, digits), seq=_seq(rng, 33), qual="*",
                                                                   aux=["NM:i:1"])))
    out.append(("cigar_max_length", line("cmax", pos=1, cigar="268435455M", seq="ACGT", qual="!!!!")))
    out.append(("cigar65535", line("c65535", pos=2000, cigar="1M1I" * 32767 + "1M", seq=_seq(rng, 50), qual="*", aux=["NM:i:7", "XS:Z:tail"])))
    out.append(("cigar65536", line("c65536", pos=3000, cigar="2M1D" * 32768, seq=_seq(rng, 51), qual=_qual(rng, 51), aux=["NM:i:8", "XS:Z:tail", "XF:f:1e-40"])))
    for v in INTS:
        out.append(("int%d" % v, line("i", pos=9, seq="ACG", qual="III", cigar="3M", aux=["XI:i:%d" % v, "XJ:i:+%d" % abs(v) if v >= 0 else "XJ:i:%d" % v])))
    out.append(("floats_fast", line("ff", pos=10, cigar="2M", seq="AC", qual="*", aux=["F%s:f:%s" % ("abcdefghijklmnopqrstuvwxyz"[j], t) for j, t in enumerate(FAST_FLOATS)])))
    out.append(("floats_slow", line("fs", pos=11, cigar="2M", seq="AC", qual="*", aux=["S%s:f:%s" % ("abcdefghijklmnopqrstuvwxyz"[j], t) for j, t in enumerate(SLOW_FLOATS)])))
    sa = ";".join("chr%d,%d,%s,%dM%dS,%d,%d" % (1 + j % 2, 1000 + 37 * j, "+-"[j & 1], 100 + j, 50 + j, 60 - j % 7, j % 5) for j in range(200)) + ";"
    assert len(sa) > 5000
    out.append(("aux_kinds", line("aux", flag=2048, pos=77, cigar="10M", seq=_seq(rng, 10), qual=_qual(rng, 10),
                                  aux=["XA:A:q", "XH:H:1AE301", "XZ:Z:", "SA:Z:" + sa, "Xc:B:c,-128,127,0", "XC:B:C,0,255", "Xs:B:s,-32768,32767", "XS:B:S,65535,0,1",
                                       "Xi:B:i,-2147483648,2147483647", "XI:B:I,4294967295,0", "Xf:B:f,1.5,-0.25,1e-40,inf,3", "XE:B:c", "Xe:B:f", "ZZ:Z:the end"])))
    out.append(("many_tags", line("many", pos=78, cigar="4M", seq="ACGT", qual="*", aux=["%s%s:i:%d" % ("ABCDEFGHIJ"[j // 10], "0123456789"[j % 10], j * 977 - 40000) for j in range(100)])))
    out.append(("no_aux", line("plain", pos=79, cigar="4M", seq="ACGT", qual="IIII")))
    out.append(("rname_star", line("unplaced", flag=4, rname="*", pos=0, mapq=0, seq="ACGTN", qual="*")))
    out.append(("unmapped_with_position_zero", line("um0", flag=4, rname="chr2", pos=0, mapq=0, seq="ACG", qual="!!~")))
    out.append(("rnext_equal", line("mate", flag=99, rname="chr2", pos=500, cigar="5M", rnext="=", pnext=900, tlen=405, seq="ACGTA", qual="*")))
    out.append(("rnext_name_tlen_min", line("mate2", flag=147, rname="chr2", pos=2 ** 31 - 1, cigar="5M", rnext="chrM_long_name", pnext=2 ** 31 - 1, tlen=-2 ** 31, seq="ACGTA", qual="*")))
    out.append(("tlen_max_star_qname", line("*", flag=65535, rname="chrM_long_name", pos=16569, mapq=255, cigar="3S", rnext="*", pnext=0, tlen=2 ** 31 - 1, seq="ACG", qual="*")))
    out.append(("cigar_without_reference_bases", line("clip", pos=4242, cigar="5S3I", seq="ACGTACGT", qual="*")))
    return out


def text(case_lines=None, last_newline=True, header=HEADER):
    ls = [l for _, l in (lines() if case_lines is None else case_lines)]
    body = b"\n".join(ls) + (b"\n" if last_newline and ls else b"")
    return header + body


def n_slow_floats(case_lines):
    """floats of the lines that miss the fast path, by the definition's own rule"""
    from svim_amd import sam
    n = 0
    for _, l in case_lines:
        for fld in l.split(b"\t")[11:]:
            if fld[3:4] == b"f":
                n += 0 if sam.float_fast_path(fld[5:]) else 1
            elif fld[3:6] == b"B:f":
                n += sum(0 if sam.float_fast_path(v) else 1 for v in fld[5:].split(b",")[1:])
    return n


E_ARG, E_RANGE = -3, -10
GOOD = dict(qname="bad", pos=10, cigar="4M", seq="ACGT", qual="IIII")


def refusals():
    """[(name, line, status)]: each line breaks one rule"""
    g = GOOD
    return [
        ("ten_fields", b"\t".join(line(**g).split(b"\t")[:10]), E_ARG),
        ("empty_line", b"", E_ARG),
        ("flag_out_of_range", line(flag=65536, **g), E_RANGE),
        ("flag_not_a_number", line(flag="0x10", **g), E_RANGE),
        ("pos_negative", line(**dict(g, pos=-1)), E_RANGE),
        ("pos_beyond_int32", line(**dict(g, pos=2 ** 31)), E_RANGE),
        ("mapq_256", line(mapq=256, **g), E_RANGE),
        ("tlen_beyond_int32", line(tlen=2 ** 31, **g), E_RANGE),
        ("overlong_number", line(tlen="1" + "0" * 30, **g), E_RANGE),
        ("pnext_empty", line(pnext="", **g), E_RANGE),
        ("unknown_rname", line(rname="chrUn", **g), E_ARG),
        ("unknown_rnext", line(rnext="chrUn", **g), E_ARG),
        ("cigar_bad_letter", line(**dict(g, cigar="4Q")), E_ARG),
        ("cigar_without_length", line(**dict(g, cigar="M")), E_ARG),
        ("cigar_trailing_digits", line(**dict(g, cigar="4M3")), E_ARG),
        ("cigar_length_beyond_28_bits", line(**dict(g, cigar="268435456M")), E_ARG),
        ("cigar_ten_digits", line(**dict(g, cigar="0000000004M")), E_ARG),
        ("qual_shorter_than_seq", line(**dict(g, qual="III")), E_ARG),
        ("qname_255", line(**dict(g, qname="q" * 255)), E_ARG),
        ("qname_empty", line(**dict(g, qname="")), E_ARG),
        ("aux_bad_type", line(aux=["XX:Q:1"], **g), E_ARG),
        ("aux_too_short", line(aux=["XX:i"], **g), E_ARG),
        ("aux_int_beyond_uint32", line(aux=["XX:i:4294967296"], **g), E_RANGE),
        ("aux_int_below_int32", line(aux=["NM:i:1", "XX:i:-2147483649"], **g), E_RANGE),
        ("aux_A_two_bytes", line(aux=["XX:A:ab"], **g), E_ARG),
        ("aux_B_bad_subtype", line(aux=["XX:B:x,1"], **g), E_ARG),
        ("aux_B_value_out_of_range", line(aux=["XX:B:c,128"], **g), E_RANGE),
        ("aux_B_empty_value", line(aux=["XX:B:s,1,,2"], **g), E_RANGE),
        ("aux_float_not_a_number", line(aux=["XX:f:1.5x"], **g), E_ARG),
        # what float() or strtod would take and the float grammar does not
        ("aux_float_leading_blank", line(aux=["XX:f: 1.5"], **g), E_ARG),
        ("aux_float_underscore", line(aux=["XX:f:1_0"], **g), E_ARG),
        ("aux_float_hexadecimal", line(aux=["XX:f:0x1p3"], **g), E_ARG),
        ("aux_float_nan_with_payload", line(aux=["XX:B:f,1,nan(1)"], **g), E_ARG),
        ("aux_float_exponent_without_digits", line(aux=["XX:f:1e"], **g), E_ARG),
        ("aux_trailing_tab", line(**g) + b"\t", E_ARG),
        ("header_after_alignment", b"@CO\tlate", E_ARG),
    ]


def several_faults():
    """[(name, lines, index of the line that is reported, status)]: more than one fault in a text or in a line.  The first bad line is reported, and within a
    line the first fault in the order svim_amd/sam.py states - whichever pass of a build finds which fault"""
    g, ok = GOOD, line(**GOOD)
    bad_flag, bad_aux, bad_ref, bad_float = line(flag=65536, **g), line(aux=["XX:Q:1"], **g), line(rname="chrUn", **g), line(aux=["XX:f:1.5x"], **g)
    return [
        ("fixed_field_before_aux", [ok, bad_flag, ok, bad_aux, ok], 1, E_RANGE),
        ("aux_before_fixed_field", [ok, bad_aux, ok, bad_flag], 1, E_ARG),
        ("reference_before_cigar", [bad_ref, line(**dict(g, cigar="4Q"))], 0, E_ARG),
        ("float_before_fixed_field", [ok, ok, bad_float, bad_flag], 2, E_ARG),
        ("fixed_field_before_float", [ok, bad_flag, bad_float], 1, E_RANGE),
        ("one_line_cigar_then_aux_integer", [ok, line(aux=["XX:i:4294967296"], **dict(g, cigar="4Q"))], 1, E_ARG),
        ("one_line_aux_type_then_flag", [ok, line(flag=65536, aux=["XX:Q:1"], **g)], 1, E_ARG),
        ("one_line_flag_then_float", [ok, line(flag=65536, aux=["XX:f:1.5x"], **g)], 1, E_RANGE),
        ("one_line_aux_integer_then_earlier_float", [ok, line(aux=["XX:f:1.5x", "XY:i:4294967296"], **g)], 1, E_RANGE),
        ("one_line_flag_then_reference", [line(flag=65536, rname="chrUn", **g)], 0, E_RANGE),
    ]


def seeded_file(seed, n):
    """header + n alignment lines of the everyday kind: a few operations, qualities, the tags an aligner writes, some split reads, any order"""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        ls = rng.choice((0, 1, 30, 75, 150, 151, 400)) if k % 50 == 0 else rng.randrange(40, 260)
        n_ops = rng.randrange(1, 12)
        cig, left = [], ls
        for j in range(n_ops):
            take = left if j == n_ops - 1 else rng.randrange(0, left + 1)
            left -= take
            if take:
                cig.append("%d%s" % (take, rng.choice("MIS=X")))
            if rng.random() < 0.3:
                cig.append("%d%s" % (rng.randrange(1, 3000), rng.choice("DN")))
        unmapped = rng.random() < 0.03
        aux = ["NM:i:%d" % rng.randrange(0, 70000), "AS:i:%d" % -rng.randrange(0, 40000), "de:f:%.4f" % rng.random(), "tp:A:%s" % rng.choice("PS")]
        if rng.random() < 0.1:
            aux.append("SA:Z:%s,%d,%s,%dM%dS,%d,%d;" % (rng.choice(REFS), rng.randrange(1, 10000), rng.choice("+-"), rng.randrange(1, 200), rng.randrange(1, 200), rng.randrange(0, 61),
                                                         rng.randrange(0, 30)))
        if rng.random() < 0.05:
            aux.append("dv:f:%r" % (rng.random() * 10 ** rng.randrange(-30, 30)))
        rname = "*" if unmapped and rng.random() < 0.5 else rng.choice(REFS)
        out.append(line("read%d/%d" % (rng.randrange(0, n // 2 + 1), seed), flag=(4 if unmapped else rng.choice((0, 16, 256, 272, 2048, 2064))), rname=rname,
                        pos=0 if rname == "*" else rng.randrange(1, LENS[TID[rname]]), mapq=rng.randrange(0, 61), cigar="*" if (unmapped or not cig or ls == 0) else "".join(cig),
                        rnext=rng.choice(("*", "=")) if rname != "*" else "*", pnext=rng.randrange(0, 1000), tlen=rng.randrange(-500, 500),
                        seq=_seq(rng, ls, "ACGTN") if ls else "*", qual=_qual(rng, ls) if (ls and rng.random() < 0.9) else "*", aux=aux))
    return HEADER + b"\n".join(out) + b"\n", out
