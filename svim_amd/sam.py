"""SAM text to BAM records: the definition the device build (csrc/sam.hip, a front end of the device reader) and the host build (csrc/sam_host.cpp) are held
against.  Pure Python, no GPU, no library.  It follows the SAM specification (1.4 the alignment line, 4.2 the BAM record, 4.2.4 the aux fields) and what
htslib's parser does where the specification leaves a choice; the one deliberate difference is named under "refusals".

What the record of a line is (record_bytes; every integer little-endian):
  block_size  the bytes that follow it.
  fixed       QNAME is written NUL-terminated and may be 1 to 254 bytes; "*" is kept as a name.  RNAME "*" gives refID -1; RNEXT "=" gives the record's refID
              and "*" gives -1.  POS and PNEXT (0 .. 2^31 - 1) are stored minus 1.  FLAG is 0 .. 65535, MAPQ 0 .. 255, TLEN signed 32-bit.
  CIGAR       "*" has 0 operations.  An operation is 1 to 9 digits, at most 2^28 - 1, and a letter of "MIDNSHP=X"; it is stored as length << 4 | index.
  SEQ         "*" gives l_seq 0.  Otherwise l_seq is its length and it is packed 4 bits per base through "=ACMGRSVTWYHKDBN", case ignored, every other byte
              15; an odd tail has a zero low nibble.
  QUAL        "*" gives l_seq bytes of 0xFF.  Otherwise every byte is stored minus 33 and the length must equal l_seq.
  bin         reg2bin(pos, end) with end = pos + the reference length of the CIGAR (operations M, D, N, =, X); when the record is unmapped (flag 4) or that
              length is 0, end = pos + 1 - which gives 4680 at pos = -1.
  long CIGAR  beyond 65 535 operations the record holds the two operations <l_seq>S<reflen>N and the real CIGAR follows as CG:B:I behind the last aux field.
  aux         A, Z and H are stored as written (Z and H NUL-terminated).  i takes the smallest type that holds the value: negative values c from -128, s from
              -32768, then i; non-negative values C to 255, S to 65535, then I; the value lies in -2^31 .. 2^32 - 1.  f is (float)strtod(text): the text's
              nearest double, then that double's nearest float - rounded twice, as htslib's is; here struct.pack('<f', float(text)), +-inf beyond float's
              range.  The text of a float is [+-] (digits [. [digits]] | . digits) [(e|E) [+-] digits], or [+-] inf, infinity or nan in either case: what
              strtod and float() both take.  Blanks, underscores, hexadecimal floats and "nan(...)" are refused.  B:<t>,v,v,.. is the
              subtype, a 32-bit count and the values, each within its subtype's range; "B:<t>" alone is an empty array.
  refusals    SamError with the 1-based line number: fewer than 11 fields (E_ARG), a number that is missing, malformed or out of its field's range
              (E_RANGE), a bad aux field or type, a bad CIGAR, a QUAL whose length differs from SEQ's, a QNAME that is empty or too long, a header line after
              the first alignment, and an RNAME or RNEXT that the dictionary does not hold (all E_ARG).  htslib warns about an unknown reference name and
              writes -1; refusing it is deliberate - a record that has silently lost its contig would be sorted and indexed as unplaced.
              A line with several faults is refused for the first of: header line, field count, QNAME, empty SEQ or QUAL, QUAL length, CIGAR, the aux
              fields from left to right, FLAG, POS, MAPQ, PNEXT, TLEN, RNAME, RNEXT, and last an 'f' value outside the float grammar.  A text is
              refused for its first bad line.
              Not checked: that the CIGAR's query length equals l_seq.

The header (header_bytes): magic, l_text, the text verbatim, n_ref and the dictionary of the @SQ lines in order (l_name, name NUL-terminated, LN).  A file with
alignment lines and no @SQ line is refused.

Floats have a fast path in the builds (float_fast_path): at most 15 significant digits m and a decimal exponent k of at most 22 in magnitude.  m and 10^|k| are
exact doubles, so m * 10^k (or m / 10^-k) is a single correctly rounded operation - the double strtod returns.  Everything else is resolved by strtod on the
host; the result is the same either way, only the builds' count of patched floats tells them apart."""
import re
import struct

E_ARG, E_RANGE = -3, -10
NT16 = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
MAX_BAM_OPS = 65535
_NIB = [15] * 256
for _i, _c in enumerate(NT16):
    _NIB[ord(_c)] = _i
    _NIB[ord(_c.lower())] = _i
_INT = re.compile(rb"[+-]?[0-9]+\Z")
_CIG = re.compile(rb"([0-9]{1,9})([MIDNSHP=X])")
_FLOAT = re.compile(rb"[+-]?(?:(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|(?i:inf|infinity|nan))\Z")
_B_RANGE = {"c": (-128, 127, "b"), "C": (0, 255, "B"), "s": (-32768, 32767, "h"), "S": (0, 65535, "H"), "i": (-2 ** 31, 2 ** 31 - 1, "i"),
            "I": (0, 2 ** 32 - 1, "I")}


class SamError(ValueError):
    """the line cannot be converted (.code E_ARG or E_RANGE, .line the 1-based line number when known)"""

    def __init__(self, code, msg, line=0):
        ValueError.__init__(self, ("line %d: " % line if line else "") + msg)
        self.code, self.line = code, line


class SamFloatError(SamError):
    """an 'f' value outside the float grammar: the last thing a line is refused for (the builds find it when they resolve the floats left to strtod)"""


def _int(text, lo, hi, what):
    if not _INT.match(text) or len(text.lstrip(b"+-").lstrip(b"0")) > 18:
        raise SamError(E_RANGE, "%s: not an integer" % what)
    v = int(text)
    if v < lo or v > hi:
        raise SamError(E_RANGE, "%s out of range" % what)
    return v


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def float_fast_path(text):
    """True when the builds convert this float text themselves (see above); False when they leave it to strtod"""
    s = bytes(text)
    i, n = 0, len(s)
    if n and s[0] in b"+-":
        i = 1
    m = nd = frac = 0
    seen = False
    while i < n and 48 <= s[i] <= 57:
        seen = True
        if m or s[i] != 48:
            nd += 1
            m = m * 10 + s[i] - 48
        i += 1
    if i < n and s[i] == 46:
        i += 1
        while i < n and 48 <= s[i] <= 57:
            seen = True
            frac += 1
            if frac > 400:
                return False
            if m or s[i] != 48:
                nd += 1
                m = m * 10 + s[i] - 48
            i += 1
    if not seen or nd > 15:
        return False
    e = 0
    if i < n and s[i] in b"eE":
        i += 1
        neg = False
        if i < n and s[i] in b"+-":
            neg = s[i] == 45
            i += 1
        j = i
        while i < n and 48 <= s[i] <= 57:
            i += 1
        if i == j or i - j > 6:
            return False
        e = -int(s[j:i]) if neg else int(s[j:i])
    if i != n:
        return False
    return -22 <= e - frac <= 22


def _float(text):
    """the 4 bytes of an 'f' value.  The grammar (_FLOAT, stated at the top) is narrower than float()'s and strtod's on purpose, so that every build can hold
    to it; a double beyond float's range is +-inf after the cast, as (float)strtod(text) is"""
    if not _FLOAT.match(text):
        raise SamFloatError(E_ARG, "bad float value")
    v = float(text.decode("ascii"))
    try:
        return struct.pack("<f", v)
    except OverflowError:
        return struct.pack("<f", float("inf") if v > 0 else float("-inf"))


def int_type(v):
    """the aux type an 'i' value is stored with, and its struct code"""
    if v < 0:
        return ("c", "b") if v >= -128 else ("s", "h") if v >= -32768 else ("i", "i")
    return ("C", "B") if v <= 255 else ("S", "H") if v <= 65535 else ("I", "I")


def aux_bytes(field, lenient=False):
    """the bytes of one aux field.  lenient: an 'f' value outside the float grammar counts as 0 (record_bytes: what else is wrong with the field comes first)"""
    flt = (lambda t: _float(t) if _FLOAT.match(t) else b"\0\0\0\0") if lenient else _float
    if len(field) < 5 or field[2:3] != b":" or field[4:5] != b":":
        raise SamError(E_ARG, "bad aux field")
    tag, ty, val = field[:2], field[3:4].decode("latin-1"), field[5:]
    if ty == "A":
        if len(val) != 1:
            raise SamError(E_ARG, "bad aux field")
        return tag + b"A" + val
    if ty in "ZH":
        return tag + ty.encode() + val + b"\0"
    if ty == "i":
        v = _int(val, -2 ** 31, 2 ** 32 - 1, "aux integer")
        t, code = int_type(v)
        return tag + t.encode() + struct.pack("<" + code, v)
    if ty == "f":
        if not val:
            raise SamError(E_RANGE, "empty float")
        return tag + b"f" + flt(val)
    if ty == "B":
        sub = val[:1].decode("latin-1")
        if sub not in "cCsSiIf" or not sub or (len(val) > 1 and val[1:2] != b","):
            raise SamError(E_ARG, "bad aux array")
        items = val[2:].split(b",") if len(val) > 1 else []
        out = [tag + b"B" + sub.encode() + struct.pack("<I", len(items))]
        for it in items:
            if not it:
                raise SamError(E_RANGE, "empty array value")
            if sub == "f":
                out.append(flt(it))
            else:
                lo, hi, code = _B_RANGE[sub]
                out.append(struct.pack("<" + code, _int(it, lo, hi, "aux array value")))
        return b"".join(out)
    raise SamError(E_ARG, "bad aux type")


def parse_cigar(text):
    if text == b"*":
        return []
    ops, at = [], 0
    for m in _CIG.finditer(text):
        if m.start() != at:
            break
        n = int(m.group(1))
        if n > 2 ** 28 - 1:
            raise SamError(E_ARG, "CIGAR length beyond 2^28 - 1")
        ops.append((n << 4) | CIGAR_OPS.index(m.group(2).decode()))
        at = m.end()
    if at != len(text) or not text:
        raise SamError(E_ARG, "bad CIGAR")
    return ops


def record_bytes(line, name_to_tid):
    """the BAM record (block_size included) of one alignment line (bytes, with or without its newline)"""
    line = bytes(line)
    if line.endswith(b"\n"):
        line = line[:-1]
    if line[:1] == b"@":
        raise SamError(E_ARG, "header line after the first alignment")
    f = line.split(b"\t")
    if len(f) < 11:
        raise SamError(E_ARG, "fewer than 11 fields")
    qname, rname, cigar, rnext, seq, qual = f[0], f[2], f[5], f[6], f[9], f[10]
    if not 1 <= len(qname) <= 254:
        raise SamError(E_ARG, "QNAME empty or longer than 254 bytes")
    if not seq or not qual:
        raise SamError(E_RANGE, "empty SEQ or QUAL")
    l_seq = 0 if seq == b"*" else len(seq)
    if qual != b"*" and len(qual) != l_seq:
        raise SamError(E_ARG, "QUAL and SEQ differ in length")
    ops = parse_cigar(cigar)
    aux, bad_float = [], None
    for x in f[11:]:
        try:
            aux.append(aux_bytes(x))
        except SamFloatError as e:          # reported behind everything else that may be wrong with the line; until then the field only has to be well formed
            bad_float = bad_float or e
            aux_bytes(x, lenient=True)
    flag = _int(f[1], 0, 65535, "FLAG")
    pos = _int(f[3], 0, 2 ** 31 - 1, "POS") - 1
    mapq = _int(f[4], 0, 255, "MAPQ")
    pnext = _int(f[7], 0, 2 ** 31 - 1, "PNEXT") - 1
    tlen = _int(f[8], -2 ** 31, 2 ** 31 - 1, "TLEN")

    def tid_of(name):
        name = name.decode("latin-1")
        if name not in name_to_tid:
            raise SamError(E_ARG, "reference name %r is not in the @SQ dictionary" % name)
        return name_to_tid[name]
    if not rname or not rnext:
        raise SamError(E_ARG, "empty reference name")
    tid = -1 if rname == b"*" else tid_of(rname)
    ntid = tid if rnext == b"=" else -1 if rnext == b"*" else tid_of(rnext)
    if bad_float is not None:
        raise bad_float
    reflen = sum(w >> 4 for w in ops if (w & 15) in (0, 2, 3, 7, 8))
    end = pos + 1 if (flag & 4) or reflen == 0 else pos + reflen
    tail = b""
    if len(ops) > MAX_BAM_OPS:
        tail = b"CGBI" + struct.pack("<I", len(ops)) + struct.pack("<%dI" % len(ops), *ops)
        ops = [(l_seq << 4) | 4, ((reflen << 4) & 0xffffffff) | 3]
    packed = bytearray((l_seq + 1) // 2)
    if l_seq:
        nib = [_NIB[c] for c in seq]
        if l_seq & 1:
            nib.append(0)
        packed = bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(nib), 2))
    q = b"\xff" * l_seq if qual == b"*" else bytes((c - 33) & 0xff for c in qual)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qname) + 1, mapq, reg2bin(pos, end) & 0xffff, len(ops), flag, l_seq, ntid, pnext, tlen) + qname + b"\0" + \
        struct.pack("<%dI" % len(ops), *ops) + bytes(packed) + q + b"".join(aux) + tail
    return struct.pack("<I", len(body)) + body


def split_text(text):
    """SAM text -> (header text, [alignment lines without their newlines]); the header is every leading line that starts with '@'"""
    text = bytes(text)
    p = 0
    while text[p:p + 1] == b"@":
        e = text.find(b"\n", p)
        p = len(text) if e < 0 else e + 1
    body = text[p:]
    lines = body.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return text[:p], lines


def dictionary(header_text):
    """[(name, length)] of the @SQ lines in order"""
    out = []
    for ln in bytes(header_text).split(b"\n"):
        if ln.startswith(b"@SQ\t"):
            d = dict((x[:2], x[3:]) for x in ln.split(b"\t")[1:] if x[2:3] == b":")
            if b"SN" not in d or b"LN" not in d:
                raise SamError(E_ARG, "@SQ line without SN or LN")
            out.append((d[b"SN"].decode("latin-1"), _int(d[b"LN"], 0, 2 ** 31 - 1, "LN")))
    return out


def header_bytes(header_text, have_alignments=False):
    """the BAM header of a SAM header text"""
    header_text = bytes(header_text)
    sq = dictionary(header_text)
    if have_alignments and not sq:
        raise SamError(E_ARG, "alignment lines but no @SQ line")
    out = [b"BAM\1", struct.pack("<i", len(header_text)), header_text, struct.pack("<i", len(sq))]
    for name, ln in sq:
        nm = name.encode("latin-1") + b"\0"
        out.append(struct.pack("<i", len(nm)) + nm + struct.pack("<i", ln))
    return b"".join(out)


def convert(text):
    """SAM text -> (BAM header bytes, [record bytes per alignment line]); SamError carries the line number within the text"""
    head, lines = split_text(text)
    n_head = head.count(b"\n") + (1 if head and not head.endswith(b"\n") else 0)
    tid = {n: i for i, (n, _) in enumerate(dictionary(head))}
    recs = []
    for k, ln in enumerate(lines):
        try:
            recs.append(record_bytes(ln, tid))
        except SamError as e:
            raise SamError(e.code, str(e), n_head + k + 1)
    return header_bytes(head, bool(lines)), recs


def line_of_record(rec, references):
    """the inverse, for tools and tests: one BAM record (block_size included) -> its SAM line (bytes, no newline).  Integers of every width come back as i;
    floats are written with repr of the float32's double, which converts back to the same float; a CG:B:I behind a placeholder is restored as the CIGAR"""
    import numpy as np
    rec = bytes(rec)
    tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, ntid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    p = 36
    qname = rec[p:p + l_name - 1]
    p += l_name
    ops = list(struct.unpack_from("<%dI" % n_cig, rec, p))
    p += 4 * n_cig
    packed = np.frombuffer(rec, dtype=np.uint8, count=(l_seq + 1) // 2, offset=p)
    p += (l_seq + 1) // 2
    nt = np.frombuffer(NT16.encode(), dtype=np.uint8)
    seq = np.stack([nt[packed >> 4], nt[packed & 15]], axis=1).reshape(-1)[:l_seq].tobytes() if l_seq else b"*"
    q = np.frombuffer(rec, dtype=np.uint8, count=l_seq, offset=p)
    p += l_seq
    qual = b"*" if (l_seq == 0 or (q == 0xff).all()) else (q + 33).astype(np.uint8).tobytes()
    aux = []
    while p < len(rec):
        tag, ty = rec[p:p + 2], rec[p + 2:p + 3]
        p += 3
        if ty == b"A":
            aux.append(tag + b":A:" + rec[p:p + 1])
            p += 1
        elif ty in (b"Z", b"H"):
            e = rec.index(b"\0", p)
            aux.append(tag + b":" + ty + b":" + rec[p:e])
            p = e + 1
        elif ty == b"f":
            aux.append(tag + b":f:" + repr(struct.unpack_from("<f", rec, p)[0]).encode())
            p += 4
        elif ty == b"B":
            sub = rec[p:p + 1].decode()
            n, = struct.unpack_from("<I", rec, p + 1)
            code = "f" if sub == "f" else _B_RANGE[sub][2]
            vals = struct.unpack_from("<%d%s" % (n, code), rec, p + 5)
            p += 5 + n * struct.calcsize(code)
            if tag == b"CG" and sub == "I" and n_cig == 2 and ops[0] == ((l_seq << 4) | 4) and (ops[1] & 15) == 3 and n > MAX_BAM_OPS and p == len(rec):
                ops = list(vals)
                continue
            aux.append(tag + b":B:" + sub.encode() + b"".join(b"," + (repr(v) if sub == "f" else str(v)).encode() for v in vals))
        else:
            code = {b"c": "b", b"C": "B", b"s": "h", b"S": "H", b"i": "i", b"I": "I"}[ty]
            aux.append(tag + b":i:" + str(struct.unpack_from("<" + code, rec, p)[0]).encode())
            p += struct.calcsize(code)
    cigar = "".join("%d%s" % (w >> 4, CIGAR_OPS[w & 15]) for w in ops).encode() if ops else b"*"
    ref = lambda t: b"*" if t < 0 else references[t].encode("latin-1")          # noqa: E731
    rnext = b"=" if (ntid >= 0 and ntid == tid) else ref(ntid)
    return b"\t".join([qname, str(flag).encode(), ref(tid), str(pos + 1).encode(), str(mapq).encode(), cigar, rnext, str(npos + 1).encode(), str(tlen).encode(), seq, qual] + aux)
