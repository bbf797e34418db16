"""Builders for the spilled coordinate sort (svx_bam_sort_begin_spill; svim_amd/bamsort.py: runs_of, merge_runs, piece_cuts): seeded cut sets for the CPU tests
and directed BAM files for the GPU tests, on top of tests/bam_sort_cases.py.

The directed files are made of records of one size (44 bytes: tiny_record with a 7-digit name, numbered in file order) and their BGZF blocks are cut at
record starts every `group` records, so that a reader that loads one block per chunk (SVX_BAM_DEV_CHUNK_BLOCKS=1) forms slabs of one size S = 44 * group: with
max_bytes = S every chunk is a run of its own, with max_bytes = 2 S every two chunks.  dict(path, header, records, n_ref, group, limit: max_bytes in units of
the largest chunk (None: the test's k rule), n_runs: the runs that must result (None: only more than `min_runs`), piece_blocks).

Test infrastructure only."""
import os
import random

import bai_cases as BC
import bam_sort_cases as SC
import foreign_bam as FB

REC = 44


def tiny(serial, tid, pos, flag=0):
    r = SC.tiny_record("%07d" % serial, tid, pos, flag)
    assert len(r) == REC
    return r


def cut_sets(n, seed):
    """run ends for n records: every single cut point, seeded sets of 2, 3 and n runs, and sets with empty runs"""
    rng = random.Random(seed)
    out = [[c, n] for c in range(n + 1)]
    for k in (2, 3):
        for _ in range(3):
            out.append(sorted(rng.randrange(n + 1) for _ in range(k - 1)) + [n])
    out.append(list(range(1, n + 1)))                                       # one record per run
    if n:
        c = rng.randrange(n + 1)
        out += [[0, 0, c, c, c, n, n], [n, n], [0, n]]                          # empty runs in front, inside and behind
    else:
        out += [[], [0], [0, 0, 0]]
    return out


def few_cut_sets(n, seed):
    """the cut sets without the sweep over every cut point"""
    rng = random.Random(seed)
    return [[n], [rng.randrange(n + 1), n], sorted(rng.randrange(n + 1) for _ in range(2)) + [n], list(range(1, n + 1)), [0, 0, n // 2, n // 2, n, n]] if n else [[], [0], [0, 0]]


def build_directed(dirpath):
    out = {}

    def add(name, recs, group, limit=1, n_runs=None, min_runs=2, piece_blocks=4096, starts_of_blocks=None):
        hdr = SC.header()
        path = os.path.join(dirpath, name + ".bam")
        if starts_of_blocks is None:
            cuts = lambda n_bytes, starts: starts[::group]                    # noqa: E731
        else:
            cuts = lambda n_bytes, starts: [starts[k] for k in starts_of_blocks]      # noqa: E731
        SC.write_raw(path, hdr, recs, cuts)
        out[name] = dict(path=path, header=hdr, records=list(recs), n_ref=len(SC.REFS), group=group, limit=limit, n_runs=n_runs, min_runs=min_runs, piece_blocks=piece_blocks)

    # stability across runs: 300 records over 5 keys, names numbered in file order, a run every 5 records
    keys = [(1, 700, 0), (1, 700, 16), (3, 5, 0), (1, 90000, 16), (-1, -1, 4)]
    rng = random.Random(201)
    add("five_keys_300_names", [tiny(k, *rng.choice(keys)) for k in range(300)], 5, n_runs=60)
    # a run of exactly one record: one block holds a single record as long as five
    rng = random.Random(202)
    recs = [tiny(k, rng.choice((0, 1, 3)), rng.randrange(0, 5000), rng.choice((0, 16))) for k in range(100)]
    one = SC.tiny_record("x" * (5 * REC - 37), 1, 2500, 0)
    assert len(one) == 5 * REC
    blocks = list(range(0, 50, 5)) + [50] + list(range(51, 101, 5))
    add("run_of_one_record", recs[:50] + [one] + recs[50:], 5, n_runs=21, starts_of_blocks=blocks)
    # a run of only unplaced records, in the middle of the file
    add("run_of_unplaced_records", recs[:50] + [tiny(900 + k, -1, -1, 4 | (16 if k & 1 else 0)) for k in range(5)] + recs[50:], 5, n_runs=21)
    # in order, reversed, shuffled: 6000 records in runs of 1000, pieces of one block (the stream is a little over four blocks)
    rng = random.Random(203)
    pos, asc = 0, []
    for k in range(6000):
        pos += rng.randrange(0, 3)
        asc.append((1 + (k >= 3000), pos, 0))
    add("in_order_one_run_per_piece", [tiny(k, *a) for k, a in enumerate(asc)], 1000, n_runs=6, piece_blocks=1)
    add("reverse_order", [tiny(k, *a) for k, a in enumerate(asc[::-1])], 1000, n_runs=6, piece_blocks=1)
    add("shuffled_every_piece_draws_on_every_run", [tiny(k, *a) for k, a in enumerate(SC.shuffled(asc, 204))], 1000, n_runs=6, piece_blocks=1)
    # the 225 kB record alone between small ones: it starts and ends a block of its own, sorts into the middle and spans several one-block pieces
    long_rec = FB.record_bytes(BC.seg("long", 1, 5000, [(0, 150000)], flag=16), [], qual=bytes(30 + k % 11 for k in range(150000)))
    rng = random.Random(205)
    small = [tiny(k, 1, rng.randrange(0, 10000), 0) for k in range(2000)]
    add("long_record_between_small_ones", small[:1000] + [long_rec] + small[1000:], 1000, min_runs=3, piece_blocks=1, starts_of_blocks=[0, 1000, 1001])
    # one run more than a wave and one more than a workgroup of the cuts kernel
    for n_runs in (70, 257):
        rng = random.Random(206 + n_runs)
        add("runs_%d" % n_runs, [tiny(k, rng.choice((0, 1, 3, -1)), rng.randrange(-1, 3000), rng.choice((0, 16))) for k in range(5 * n_runs)], 5, n_runs=n_runs)
    # the file ends exactly where a run is full: 8 chunks, two to a run
    rng = random.Random(207)
    add("end_on_a_run_edge", [tiny(k, rng.choice((0, 1)), rng.randrange(0, 500), 0) for k in range(40)], 5, limit=2, n_runs=4)
    return out
