"""Cases for the merge of several BAM files (svim_amd/bammerge.py, csrc/bamsort_host.cpp), built from the builders of tests/bam_sort_cases.py and
tests/bai_cases.py.  tests/test_bam_merge.py holds the definition and the host build to them on the CPU; every input is also written as a BAM file, for the
device build that is to follow.

    split          every corner file of bam_sort_cases dealt record by record into 2 and 3 files with the same header: the expected bytes are the existing
                   bamsort definition of the ONE file, which knows nothing of the new code.  The deal keeps records with equal keys in file order (the
                   members of one key go to the files in contiguous thirds), records with different keys interleave freely
    ties           five_keys_forty_names and forward_and_reverse_at_one_position dealt round-robin: equal keys sit in different files
    dictionaries   a second file with the first's dictionary reversed (a sorted input is unsorted after translation); a file that appends two contigs; a file
                   with n_ref = 0 and only unplaced records; a file without records and a dictionary of its own placed first, in the middle and last
    tiny           records of 36 to 40 bytes, 700 per file, non-identity maps: neighbours share aligned words
    mates          next_refID in {-1, own, other, the file's last}; out of range in a translated file (E_ARG) and in an identity-map file (verbatim)
    headers        every branch of the header rule, the expected text written out by hand
    long           the 225 kB record of record_longer_than_two_blocks in the second file under a non-identity map

A case: dict(inputs=[dict(path, header, records, n_ref)], and for the split cases one=the one-file case and origin=[original index of every global record
number]).  Test infrastructure only."""
import os
import random
import struct

import bai_cases as BC
import bam_sort_cases as SC
import foreign_bam as FB
from svim_amd import bammerge, bamsort

REFS, LENS = BC.REFS, BC.LENS
E_ARG = bamsort.E_ARG


def _input(dirpath, name, hdr, recs, n_ref, cuts=0xff00):
    path = os.path.join(dirpath, name + ".bam")
    SC.write_raw(path, hdr, recs, cuts)
    return dict(path=path, header=hdr, records=list(recs), n_ref=n_ref)


def tie_safe_deal(recs, k):
    """-> per file the original indices of its records, ascending: the members of every key, in file order, go to files of non-decreasing number - in k
    contiguous shares, or, when a key has fewer than k members, to neighbouring files that start at a file which turns with the keys"""
    groups = {}
    for i, r in enumerate(recs):
        groups.setdefault(bamsort.sort_key(r[4:]), []).append(i)
    files = [[] for _ in range(k)]
    for g, members in enumerate(groups.values()):
        c = len(members)
        for j, i in enumerate(members):
            files[j * k // c if c >= k else g % (k - c + 1) + j].append(i)
    return [sorted(f) for f in files]


def round_robin_deal(recs, k):
    return [list(range(f, len(recs), k)) for f in range(k)]


def dealt(dirpath, name, one, k, deal):
    parts = deal(one["records"], k)
    inputs = [_input(dirpath, "%s.%d_of_%d" % (name, f, k), one["header"], [one["records"][i] for i in part], one["n_ref"], cuts=1777 + 100 * f) for f, part in enumerate(parts)]
    return dict(inputs=inputs, one=one, origin=[i for part in parts for i in part])


def with_ids(rec, tid=None, mate=None):
    """a record's bytes with refID and / or next_refID replaced"""
    b = bytearray(rec)
    if tid is not None:
        struct.pack_into("<i", b, 4, tid)
    if mate is not None:
        struct.pack_into("<i", b, 24, mate)
    return bytes(b)


def renumbered(recs, new_of_old, mates=None, seed=0):
    """records built over REFS, as a file holds them whose dictionary lists REFS in another order: new_of_old[t] is that file's id of REFS[t].  mates: the
    next_refID values dealt over the records in turn (ids of that file)"""
    out = []
    for k, r in enumerate(recs):
        t, = struct.unpack_from("<i", r, 4)
        out.append(with_ids(r, new_of_old[t] if t >= 0 else -1, mates[k % len(mates)] if mates else None))
    return out


def header_of(refs, lens, text=None, pad=0):
    return SC.header(("@HD\tVN:1.6\tSO:coordinate\n" + SC.sq_lines(refs, lens)) if text is None else text, refs, lens, pad)


def build_split(dirpath):
    d = os.path.join(dirpath, "one")
    os.makedirs(d, exist_ok=True)
    out = {}
    for name, one in SC.build_all(d).items():
        for k in (2, 3):
            out["%s/%d" % (name, k)] = dealt(dirpath, name, one, k, tie_safe_deal)
    return out


def build_ties(dirpath):
    d = os.path.join(dirpath, "ties_one")
    os.makedirs(d, exist_ok=True)
    ones = SC.build_all(d)
    return {"%s/%d" % (name, k): dealt(dirpath, "ties_" + name, ones[name], k, round_robin_deal)
            for name in ("five_keys_forty_names", "forward_and_reverse_at_one_position") for k in (2, 3)}


def build_directed(dirpath):
    out = {}
    rev = list(range(len(REFS)))[::-1]                                       # the id, in a file with the reversed dictionary, of REFS[t]
    refs_r, lens_r = REFS[::-1], LENS[::-1]
    first = BC.record_bytes(BC.random_records(101, 220, (0, 1, 3, 5), LENS, n_unplaced=5))
    second = BC.record_bytes(BC.random_records(102, 230, (0, 2, 4, 5), LENS, n_unplaced=4))
    a = _input(dirpath, "dict_a", header_of(REFS, LENS), first, len(REFS), cuts=3001)
    # sorted in its own numbering (c5 first): unsorted once translated
    b_recs = renumbered(second[-4:] + second[:-4], rev, mates=(-1, 0, 3, 5))
    b_sorted = sorted(b_recs, key=lambda r: bamsort.sort_key(r[4:]))
    b = _input(dirpath, "dict_reversed", header_of(refs_r, lens_r), b_sorted, len(REFS), cuts=2500)
    out["reversed_dictionary"] = dict(inputs=[a, b])
    refs_n, lens_n = ["c2", "c0", "x0", "x1"], [LENS[2], LENS[0], 9000, 1 << 24]
    rng = random.Random(103)
    n_recs = [SC.tiny_record("n%d" % k, rng.randrange(-1, 4), rng.randrange(-1, 4000), rng.choice((0, 16))) for k in range(150)]
    n_recs = [with_ids(r, mate=m) for r, m in zip(n_recs, [(-1, 0, 2, 3)[k % 4] for k in range(150)])]
    c = _input(dirpath, "dict_appends_two", header_of(refs_n, lens_n), n_recs, 4, cuts=1500)
    out["appends_two_contigs"] = dict(inputs=[a, c])
    u_recs = BC.record_bytes([BC.seg("u%d" % k, -1, -1 if k % 3 else 50 + k, [], flag=4 | (16 if k & 1 else 0)) for k in range(40)])
    u = _input(dirpath, "dict_no_references", SC.header("@HD\tVN:1.6\tSO:unsorted\n", [], []), u_recs, 0)
    out["no_references_only_unplaced"] = dict(inputs=[a, u, b])
    e = _input(dirpath, "dict_empty", header_of(["c5", "c4", "e0"], [LENS[5], LENS[4], 777]), [], 3)
    out["empty_file_first"] = dict(inputs=[e, a, b])
    out["empty_file_in_the_middle"] = dict(inputs=[a, e, b])
    out["empty_file_last"] = dict(inputs=[a, b, e])
    # tiny records: every start alignment mod 4 and mod 16, two translated files
    rng = random.Random(104)
    tiny = lambda tag, n: [with_ids(SC.tiny_record(tag * (3 + k % 5), rng.choice((0, 1, 1, 3, 5, -1)), rng.randrange(-1, 60), rng.choice((0, 16, 4))), mate=rng.choice((-1, 0, 2, 5)))      # noqa: E731
                           for k in range(n)]
    t0 = _input(dirpath, "tiny_0", header_of(REFS, LENS), tiny("a", 90), len(REFS), cuts=997)
    t1 = _input(dirpath, "tiny_1", header_of(refs_r, lens_r), tiny("b", 700), len(REFS), cuts=997)
    t2 = _input(dirpath, "tiny_2", header_of(REFS[1:] + REFS[:1], LENS[1:] + LENS[:1]), tiny("c", 700), len(REFS), cuts=1301)
    out["tiny_records"] = dict(inputs=[t0, t1, t2])
    assert {len(r) - 4 for r in t1["records"]} == {36, 37, 38, 39, 40} and len({sum(map(len, t1["records"][:k])) % 16 for k in range(700)}) == 16
    # mate ids
    m_recs = [with_ids(r, mate=(-1, 0, 3, 5, 1, 5)[k % 6]) for k, r in enumerate(renumbered(first[:120], rev))]
    m = _input(dirpath, "mates_translated", header_of(refs_r, lens_r), m_recs, len(REFS))
    out["mate_ids_of_every_kind"] = dict(inputs=[a, m])
    for tag, bad in (("beyond", len(REFS)), ("below", -2), ("far_beyond", 1 << 30)):
        mb = _input(dirpath, "mates_bad_" + tag, header_of(refs_r, lens_r), m_recs[:50] + [with_ids(m_recs[50], mate=bad)] + m_recs[51:], len(REFS))
        out["mate_id_%s_in_a_translated_file" % tag] = dict(inputs=[a, mb], error=E_ARG)
        ident = _input(dirpath, "mates_ident_" + tag, header_of(REFS, LENS), first[:50] + [with_ids(first[50], mate=bad)] + first[51:], len(REFS))
        out["mate_id_%s_in_an_identity_file" % tag] = dict(inputs=[a, ident])
    bad_tid = _input(dirpath, "tid_bad", header_of(refs_r, lens_r), m_recs[:10] + [with_ids(m_recs[10], tid=len(REFS))], len(REFS))
    out["reference_id_beyond_in_a_translated_file"] = dict(inputs=[a, bad_tid], error=E_ARG)
    below = _input(dirpath, "pos_below", header_of(refs_r, lens_r), m_recs[:10] + [m_recs[10][:8] + struct.pack("<i", -2) + m_recs[10][12:]], len(REFS))
    out["position_below_minus_one"] = dict(inputs=[a, below], error=bamsort.E_RANGE)
    out["position_below_and_a_bad_mate"] = dict(inputs=[a, below, mb], error=E_ARG)      # E_ARG in a later file goes before E_RANGE
    # the long record
    long_rec = FB.record_bytes(BC.seg("long", rev[1], 5000, [(0, 150000)], flag=16), [], qual=bytes(30 + k % 11 for k in range(150000)))
    around = renumbered(BC.record_bytes(BC.random_records(105, 60, (1, 3), LENS, n_unplaced=2)), rev)
    lg = _input(dirpath, "long_record", header_of(refs_r, lens_r), SC.shuffled(around + [with_ids(long_rec, mate=rev[3])], 106), len(REFS), cuts=40000)
    assert len(long_rec) > 225000
    out["long_record_in_a_translated_file"] = dict(inputs=[a, lg])
    return out


SQ = SC.sq_lines()
HEADER_CASES = {
    # name: ([(text, refs, lens, pad)], the expected text's lines, or the error code)
    "no_hd_line": ([(SQ + "@PG\tID:a\n", REFS, LENS, 0), (SQ + "@CO\tsecond\n", REFS, LENS, 0)],
                   ["@HD\tVN:1.6\tSO:coordinate"] + SQ.splitlines() + ["@PG\tID:a", "@CO\tsecond"]),
    "sq_in_one_file_only": ([("@HD\tVN:1.5\tSO:unsorted\n@RG\tID:r1\n", REFS[:2], LENS[:2], 0),
                             ("@HD\tVN:1.6\n@SQ\tSN:c1\tLN:%d\tM5:abc\n@SQ\tSN:z\tLN:5\tSP:x\n" % LENS[1], ["c1", "c0", "z"], [LENS[1], LENS[0], 5], 0)],
                            ["@HD\tVN:1.5\tSO:coordinate", "@SQ\tSN:c0\tLN:%d" % LENS[0], "@SQ\tSN:c1\tLN:%d\tM5:abc" % LENS[1], "@SQ\tSN:z\tLN:5\tSP:x", "@RG\tID:r1"]),
    "sq_behind_rg": ([("@HD\tVN:1.6\tSO:queryname\tGO:query\n@RG\tID:r\tSM:s\n" + SQ + "@CO\tx\n", REFS, LENS, 0), ("@HD\tVN:1.6\n" + SQ, REFS, LENS, 0)],
                     ["@HD\tVN:1.6\tSO:coordinate"] + SQ.splitlines() + ["@RG\tID:r\tSM:s", "@CO\tx"]),
    "identical_rg_kept_once": ([("@HD\tVN:1.6\n" + SQ + "@RG\tID:r\tSM:s\n", REFS, LENS, 0), ("@HD\tVN:1.6\n" + SQ + "@RG\tID:r\tSM:s\n@RG\tID:q\tSM:s\n", REFS, LENS, 0)],
                               ["@HD\tVN:1.6\tSO:coordinate"] + SQ.splitlines() + ["@RG\tID:r\tSM:s", "@RG\tID:q\tSM:s"]),
    "conflicting_rg": ([("@HD\tVN:1.6\n" + SQ + "@RG\tID:r\tSM:s\n", REFS, LENS, 0), ("@HD\tVN:1.6\n" + SQ + "@RG\tID:r\tSM:other\n", REFS, LENS, 0)], E_ARG),
    "pg_same_id_three_files": ([("@HD\tVN:1.6\n" + SQ + "@PG\tID:x\tPN:aln\tCL:run %d\n@PG\tID:y\tPN:post\tPP:x\n" % f, REFS, LENS, 0) for f in range(3)],
                               ["@HD\tVN:1.6\tSO:coordinate"] + SQ.splitlines() +
                               ["@PG\tID:x\tPN:aln\tCL:run 0", "@PG\tID:y\tPN:post\tPP:x", "@PG\tID:x-1\tPN:aln\tCL:run 1", "@PG\tID:y-1\tPN:post\tPP:x-1",
                                "@PG\tID:x-2\tPN:aln\tCL:run 2", "@PG\tID:y-2\tPN:post\tPP:x-2"]),
    "pg_renamed_id_is_taken": ([("@HD\tVN:1.6\n" + SQ + "@PG\tID:x\tCL:a\n@PG\tID:x-1\tCL:b\n", REFS, LENS, 0), ("@HD\tVN:1.6\n" + SQ + "@PG\tID:x\tCL:c\n@PG\tID:x\tCL:a\n", REFS, LENS, 0)],
                               ["@HD\tVN:1.6\tSO:coordinate"] + SQ.splitlines() + ["@PG\tID:x\tCL:a", "@PG\tID:x-1\tCL:b", "@PG\tID:x-1-1\tCL:c"]),
    "nul_tail": ([("@HD\tVN:1.6\n" + SQ + "@CO\tone\n", REFS, LENS, 29), ("@HD\tVN:1.6\n" + SQ + "@CO\ttwo\n", REFS, LENS, 3)],
                 ["@HD\tVN:1.6\tSO:coordinate"] + SQ.splitlines() + ["@CO\tone", "@CO\ttwo"]),
    "last_line_without_newline": ([("@HD\tVN:1.6\n" + SQ + "@CO\tone", REFS, LENS, 0), ("@HD\tVN:1.6\n" + SQ + "\n\n@CO\ttwo", REFS, LENS, 0), ("@CO\tthree", [], [], 0)],
                                  ["@HD\tVN:1.6\tSO:coordinate"] + SQ.splitlines() + ["@CO\tone", "@CO\ttwo", "@CO\tthree"]),
    "no_text_anywhere": ([("", REFS[:2], LENS[:2], 0), ("", REFS[1:3], LENS[1:3], 0)], ["@HD\tVN:1.6\tSO:coordinate"]),
    "same_name_two_lengths": ([("@HD\tVN:1.6\n", REFS, LENS, 0), ("@HD\tVN:1.6\n", ["c1"], [LENS[1] + 1], 0)], E_ARG),
    "name_twice_in_one_dictionary": ([("@HD\tVN:1.6\n", REFS, LENS, 0), ("@HD\tVN:1.6\n", ["q", "c1", "q"], [5, LENS[1], 5], 0)], E_ARG),
}


def build_headers(dirpath):
    """every header case with a few records per file -> {name: dict(inputs, lines or error)}"""
    out = {}
    for name, (files, want) in HEADER_CASES.items():
        inputs = []
        for f, (text, refs, lens, pad) in enumerate(files):
            rng = random.Random(200 + f)
            recs = [SC.tiny_record("h%d_%d" % (f, k), rng.randrange(-1, len(refs)), rng.randrange(0, 900), rng.choice((0, 16))) for k in range(12)]
            inputs.append(_input(dirpath, "header_%s_%d" % (name, f), SC.header(text, refs, lens, pad), recs, len(refs)))
        out[name] = dict(inputs=inputs, **({"error": want} if isinstance(want, int) else {"lines": want}))
    return out


def build_all(dirpath):
    out = {}
    for prefix, built in (("split", build_split), ("ties", build_ties), ("directed", build_directed), ("header", build_headers)):
        d = os.path.join(dirpath, prefix)
        os.makedirs(d, exist_ok=True)
        for name, case in built(d).items():
            out["%s:%s" % (prefix, name)] = case
    return out


def raws(case):
    return [x["header"] + b"".join(x["records"]) for x in case["inputs"]]


def definition(case):
    """-> (the merged stream, the permutation) of a case by svim_amd/bammerge.py; BamMergeError for the refused ones"""
    return bammerge.stream_of(raws(case))
