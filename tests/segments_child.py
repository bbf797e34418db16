"""Child process of the mutant test (tests/test_segments.py): compares the oracle library that SVX_ORACLE_LIB names with tests/golden/g_segments_cases.json.gz.
Exit status 0: every row agrees; DIFFERENT: a difference, printed.  Anything else (an exception ends Python with 1) is a failure of the child, not a verdict."""
import os
import sys

DIFFERENT = 3


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import helpers as H
    from oracle import oracle as om
    from segment_checks import GOLDEN, golden_difference
    g = H.load(GOLDEN)
    oc = om.Oracle()
    for case in g["cases"]:
        d = golden_difference(oc, g, case)
        if d:
            print(d)
            return DIFFERENT
    return 0


if __name__ == "__main__":
    sys.exit(main())
