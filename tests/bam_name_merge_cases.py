"""Cases for the merge of several BAM files in query-name order (svim_amd/bammerge.py, order="queryname"; csrc/bamsort_host.cpp: svx_bam_merge_host_order;
csrc/bamsort.hip: runs in query-name order, k_ns_pack, k_ns_keys_tab), built on tests/bam_name_sort_cases.py and tests/bam_merge_cases.py.
tests/test_bam_name_merge.py holds the definition and the host build to them on the CPU, tests/test_gpu_bam_name_merge.py the session on the GPU.

    split          every file of bam_name_sort_cases dealt into 2 and 3 files by a tie-safe deal keyed on name_key (the members of one key go to files of
                   non-decreasing number): the expected bytes are the EXISTING bamsort definition of the one file, which knows nothing of the new code
    ties           stable_ties (5 000 equal keys) and duplicated_reads (forty_names_duplicated) dealt round-robin: equal keys sit in different files
    dictionaries   a second file with the first's dictionary reversed, a file that appends contigs: ids are translated while the key ignores them
    run edges      one file each whose BGZF blocks are GROUPS of records of one byte size (fillers pad them): a reader that loads a block at a time and an arena
                   of one group's bytes close a run after every group, so the records named below sit in different runs
                       run_edge_lengths        one stem cut to every length of LENGTHS: a name that ends on a word's edge and its one-byte-longer neighbour
                       run_edge_prefix_chain   a / ab / abc / abcd / abcde
                       run_edge_high_bytes     0x7f / 0x80 / 0xff in the deciding byte (a signed compare of table words)
                       run_edge_padded_fields  NUL inside the field, junk behind it, fields without a NUL
                       run_edge_ranks          every name_rank twice under one name, over three runs
                       run_edge_64_rounds      the pairs of 253- and 254-byte names that differ in their last byte, in two runs: 64 rounds in the merge
                       run_edge_long_record    the 225 kB record between small ones
                       run_edge_run_of_one     a run that holds one record
                       run_edge_70_runs, run_edge_257_runs
    headers        the twelve header texts of bam_merge_cases; the expected first line in query-name order written out by hand
    refused        a record without a name field in the second file (E_ARG); that together with pos < -1 in the first file (still E_ARG); pos < -1 alone (E_RANGE)

A case: dict(inputs=[dict(path, header, records, n_ref)]), for the split cases one= and origin= as in bam_merge_cases, for the run-edge cases max_bytes= (one
group) and min_runs=.  Test infrastructure only."""
import os
import random
import struct

import bai_cases as BC
import bam_merge_cases as MC
import bam_name_sort_cases as NC
import bam_sort_cases as SC
import foreign_bam as FB
from svim_amd import bammerge, bamsort

REFS, LENS = MC.REFS, MC.LENS
E_ARG, E_RANGE = bamsort.E_ARG, bamsort.E_RANGE
FIRST_LINE = "@HD\tVN:%s\tSO:queryname\tSS:queryname:lexicographical"


def tie_safe_deal(recs, k):
    """bam_merge_cases.tie_safe_deal keyed on name_key: the members of every (name, rank), in file order, go to files of non-decreasing number"""
    groups = {}
    for i, r in enumerate(recs):
        groups.setdefault(bamsort.name_key(r[4:]), []).append(i)
    files = [[] for _ in range(k)]
    for g, members in enumerate(groups.values()):
        c = len(members)
        for j, i in enumerate(members):
            files[j * k // c if c >= k else g % (k - c + 1) + j].append(i)
    return [sorted(f) for f in files]


def build_split(dirpath):
    d = os.path.join(dirpath, "one")
    os.makedirs(d, exist_ok=True)
    return {"%s/%d" % (name, k): MC.dealt(dirpath, name, one, k, tie_safe_deal) for name, one in NC.build_all(d).items() for k in (2, 3)}


def build_ties(dirpath):
    d = os.path.join(dirpath, "ties_one")
    os.makedirs(d, exist_ok=True)
    ones = NC.build_all(d)
    return {"%s/%d" % (name, k): MC.dealt(dirpath, "ties_" + name, ones[name], k, MC.round_robin_deal) for name in ("stable_ties", "duplicated_reads") for k in (2, 3)}


def build_dictionaries(dirpath):
    """reads whose records lie in several files under several dictionaries: the names repeat across the files, the ids do not mean the same anywhere"""
    rev = list(range(len(REFS)))[::-1]
    rng = random.Random(301)
    made = lambda n, tids: [NC.name_record(b"read%03d/%d" % (rng.randrange(120), rng.randrange(3)), rng.choice(tids), rng.randrange(-1, 4000), rng.choice((0, 16, 2048, 256, 64, 128 | 2048)))     # noqa: E731
                            for _ in range(n)]
    a = MC._input(dirpath, "names_dict_a", MC.header_of(REFS, LENS), made(220, (0, 1, 3, 5, -1)), len(REFS), cuts=3001)
    b = MC._input(dirpath, "names_dict_reversed", MC.header_of(REFS[::-1], LENS[::-1]), MC.renumbered(made(230, (0, 2, 4, 5)), rev, mates=(-1, 0, 3, 5)), len(REFS), cuts=2500)
    refs_n, lens_n = ["c2", "c0", "x0", "x1"], [LENS[2], LENS[0], 9000, 1 << 24]
    c_recs = [MC.with_ids(r, mate=(-1, 0, 2, 3)[k % 4]) for k, r in enumerate(made(150, (-1, 0, 1, 2, 3)))]
    c = MC._input(dirpath, "names_dict_appends_two", MC.header_of(refs_n, lens_n), c_recs, 4, cuts=1500)
    return {"reversed_dictionary": dict(inputs=[a, b]), "appends_two_contigs": dict(inputs=[a, c]), "three_dictionaries": dict(inputs=[b, c, a])}


# ---- run edges -------------------------------------------------------------------------------------------------------------------------------------------
def _fill(n_bytes, tag):
    """filler records of exactly n_bytes in all (0, or at least 38): 37 bytes and a name of 1 .. 254 bytes each"""
    out, k = [], 0
    while n_bytes > 0:
        take = n_bytes if n_bytes <= 291 else (291 if n_bytes - 291 >= 38 else n_bytes - 38)
        assert 38 <= take <= 291
        out.append(NC.name_record((b"~%s.%d." % (tag, k) + b"f" * 254)[:take - 37], 1, 7))
        n_bytes -= take
        k += 1
    return out


def equalised(groups, tag):
    """every group padded with fillers to one byte size -> (groups, that size)"""
    size = max(sum(map(len, g)) for g in groups) + 38
    return [list(g) + _fill(size - sum(map(len, g)), b"%s%d" % (tag, j)) for j, g in enumerate(groups)], size


def run_edge_case(dirpath, name, groups, max_bytes, min_runs=None):
    """one file whose BGZF blocks are the header and then one block per group (a group of more than 65 280 bytes: several)"""
    recs = [r for g in groups for r in g]
    hdr = SC.header()
    edges = []

    def cuts(total, starts):
        at, k = [len(hdr)], 0
        for g in groups:
            at.append(starts[k] if k < len(starts) else total)
            k += len(g)
        edges.extend(at)
        return at
    x = MC._input(dirpath, name, hdr, recs, len(REFS), cuts=cuts)
    sizes = [sum(map(len, g)) for g in groups]
    assert all(s <= max_bytes for s in sizes)
    return dict(inputs=[x], groups=[len(g) for g in groups], max_bytes=max_bytes, min_runs=len(runs_of_groups(sizes, max_bytes)) if min_runs is None else min_runs)


def runs_of_groups(sizes, max_bytes):
    """the runs an arena of max_bytes forms of chunks of these sizes: a chunk that does not fit closes the open run -> per run the list of its groups"""
    runs, held = [[]], 0
    for j, s in enumerate(sizes):
        if held and held + s > max_bytes:
            runs.append([])
            held = 0
        runs[-1].append(j)
        held += s
    return runs


def build_run_edges(dirpath):
    out = {}

    def add(name, groups, tag):
        groups, size = equalised(groups, tag)
        out[name] = run_edge_case(dirpath, name, groups, size)
        assert out[name]["min_runs"] == len(groups) >= 2
    rng = random.Random(311)
    stem = NC._ascii(rng, 254)
    add("run_edge_lengths", [[NC.name_record(stem[:n], rng.choice((0, 1, 3)), rng.randrange(5000))] for n in SC.shuffled(NC.LENGTHS, 312)], b"L")
    add("run_edge_prefix_chain", [[NC.name_record(n)] for n in (b"abc", b"a", b"abcde", b"ab", b"abcd")], b"P")
    add("run_edge_high_bytes", [[NC.name_record(n, flag=f) for f in (16, 0)] for n in (b"rrr\xffx", b"rrrr\x80", b"rrr\x7fx", b"rrrr\xff", b"rrr\x80x", b"rrrr\x7f", b"rrr", b"rrrr")], b"H")
    fields = [b"pad\0zzz\0", b"pad\0aaa\0", b"pad\0", b"pa\0\xff\xff\xff\xff\0", b"padd\0\0\0\0", b"pac\0dddddddd\0", b"p\0" + b"\x01" * 250 + b"\0", b"paddle\0", b"no_nul_in_the_field",
              b"no_nul_in_the_fiel\0", b"no_nul_in_the_field!\0", b"Z" * 255, b"Z" * 254 + b"\0", b"pad\0\0\0\0\0"]
    add("run_edge_padded_fields", [[NC.name_record(b"", field=f)] for f in fields], b"F")
    ranks = SC.shuffled([NC.name_record(b"one_read", k % 4, 10 * k, f | s) for k, (f, s) in enumerate((f, s) for f in NC.RANK_FLAGS for s in (0, 16))], 313)
    add("run_edge_ranks", [ranks[j::3] for j in range(3)], b"R")
    long_a, long_b = NC._ascii(rng, 252), NC._ascii(rng, 253)
    add("run_edge_64_rounds", [[NC.name_record(long_a + b"z"), NC.name_record(long_b + b"z")], [NC.name_record(long_b + b"y"), NC.name_record(long_a + b"y")]], b"W")
    # a run of one record: it has the size of a whole group, so neither neighbour fits beside it
    groups, size = equalised([[NC.name_record(b"front%02d" % k) for k in range(5)], [NC.name_record(b"back%02d" % k) for k in range(5)]], b"O")
    alone = NC.name_record((b"alone" + b"e" * 254)[:size - 37]) if size <= 291 else None
    assert alone is not None and len(alone) == size
    out["run_edge_run_of_one"] = run_edge_case(dirpath, "run_edge_run_of_one", [groups[0], [alone], groups[1]], size)
    assert out["run_edge_run_of_one"]["min_runs"] == 3
    for n_groups in (70, 257):
        add("run_edge_%d_runs" % n_groups, [[NC.name_record(b"%s/%d" % (NC._ascii(rng, rng.randrange(1, 30)), k), flag=rng.choice((0, 2048, 256))) for k in range(3)] for _ in range(n_groups)], b"N")
    # the 225 kB record between small ones: the arena holds it and one small group
    long_rec = FB.record_bytes(BC.seg("long", 1, 5000, [(0, 150000)], flag=16), [], qual=bytes(30 + k % 11 for k in range(150000)))
    assert len(long_rec) > 225000
    small, size = equalised([[NC.name_record(b"kkk%02d" % k) for k in range(6)], [NC.name_record(b"mmm%02d" % k) for k in range(6)]], b"G")
    out["run_edge_long_record"] = run_edge_case(dirpath, "run_edge_long_record", [small[0], [long_rec], small[1]], len(long_rec) + size, min_runs=2)
    return out


# ---- headers ---------------------------------------------------------------------------------------------------------------------------------------------
# the first line of the merged text in query-name order, by hand, for every accepted header case of bam_merge_cases (the lines behind it are those cases' own)
QN_FIRST_LINE = {"no_hd_line": FIRST_LINE % "1.6",                            # no @HD line: the new one
                 "sq_in_one_file_only": FIRST_LINE % "1.5",                   # SO:unsorted replaced, SS: behind it
                 "sq_behind_rg": FIRST_LINE % "1.6",                          # SO:queryname stays, GO:query goes
                 "identical_rg_kept_once": FIRST_LINE % "1.6",                # no SO: field: appended
                 "pg_same_id_three_files": FIRST_LINE % "1.6",
                 "pg_renamed_id_is_taken": FIRST_LINE % "1.6",
                 "nul_tail": FIRST_LINE % "1.6",
                 "last_line_without_newline": FIRST_LINE % "1.6",
                 "no_text_anywhere": FIRST_LINE % "1.6"}


def build_headers(dirpath):
    out = MC.build_headers(dirpath)
    for name, c in out.items():
        if "lines" in c:
            c["lines"] = [QN_FIRST_LINE[name]] + c["lines"][1:]
    return out


# ---- refused ---------------------------------------------------------------------------------------------------------------------------------------------
def build_refused(dirpath):
    """the bad record early in its file, more than 60 good records behind it; the files are cut into blocks of 600 bytes"""
    good = lambda tag, n: [NC.name_record(b"%s%03d" % (tag, k), 1, 100 + k) for k in range(n)]      # noqa: E731
    no_name = NC.name_record(b"", field=b"")
    low = NC.name_record(b"low", 1, -2)
    hdr = SC.header()
    f = lambda name, recs: MC._input(dirpath, "refused_" + name, hdr, recs, len(REFS), cuts=600)     # noqa: E731
    clean, second_bad = f("clean", good(b"a", 40)), f("no_name_second", good(b"b", 5) + [no_name] + good(b"c", 60))
    first_low = f("low_first", good(b"d", 3) + [low] + good(b"e", 60))
    return {"no_name_in_the_second_file": dict(inputs=[clean, second_bad], error=E_ARG),
            "no_name_in_the_second_file_and_pos_below_in_the_first": dict(inputs=[first_low, second_bad], error=E_ARG),
            "pos_below_minus_one_alone": dict(inputs=[first_low, clean], error=E_RANGE)}


def build_all(dirpath):
    out = {}
    for prefix, built in (("split", build_split), ("ties", build_ties), ("dict", build_dictionaries), ("edge", build_run_edges), ("header", build_headers), ("refused", build_refused)):
        d = os.path.join(dirpath, prefix)
        os.makedirs(d, exist_ok=True)
        for name, case in built(d).items():
            out["%s:%s" % (prefix, name)] = case
    return out


def raws(case):
    return MC.raws(case)


def definition(case):
    """-> (the merged stream, the permutation) of a case in query-name order by svim_amd/bammerge.py; BamMergeError for the refused ones"""
    return bammerge.stream_of(raws(case), "queryname")


def parsed(rec):
    return NC.parsed(rec)
