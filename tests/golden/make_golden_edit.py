#!/usr/bin/env python3
"""Generate tests/golden/g_edit_cases.json.gz: the plain-DP distance (tests/edit_cases.py: levenshtein_rows, a row-by-row Wagner-Fischer recurrence in integer
numpy) of every directed edit-distance case of tests/edit_cases.py.

Per case: family, name, the two lengths, the SHA-1 of both strings and the distance.  The strings are NOT stored: tests/edit_cases.py regenerates them from its
seeds and the hash catches a generator that drifted.  Needs nothing but numpy; about half a minute.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_edit.py
"""
import gzip
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edit_cases as EC    # noqa: E402


def main():
    rows = EC.golden_rows()
    fams = {}
    for r in rows:
        fams[r[0]] = fams.get(r[0], 0) + 1
    doc = {"cases": rows, "families": fams,
           "source": "unit-cost global edit distance by tests/edit_cases.py:levenshtein_rows (Wagner-Fischer, one row at a time, no bit-vectors)"}
    path = os.path.join(HERE, "g_edit_cases.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(json.dumps(doc, separators=(",", ":")).encode("ascii"))
    print(path, os.path.getsize(path), "bytes;", len(rows), "cases:", fams)


if __name__ == "__main__":
    main()
