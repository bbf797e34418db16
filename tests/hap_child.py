"""Child process of the mutant test (tests/test_hap_cases.py): compares the oracle library that SVX_ORACLE_LIB names with tests/golden/g_hap_cases.json.gz.
Exit status 0: every pair and every cluster agrees; DIFFERENT: a difference, printed.  Anything else (an exception ends Python with 1) is a failure of the child,
not a verdict."""
import os
import sys

DIFFERENT = 3


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import helpers as H
    import hap_cases as HC
    from oracle import oracle as om
    from hap_checks import GOLDEN, genome_arrays, oracle_cluster_difference, oracle_pair_difference
    g = H.load(GOLDEN)
    oc = om.Oracle()
    oc.set_genome(*genome_arrays())
    for t in HC.families():
        d = oracle_pair_difference(oc, g, t)
        if d:
            print(d)
            return DIFFERENT
    for case, (name, rows, opts) in zip(g["cluster_cases"], HC.cluster_cases()):
        d = oracle_cluster_difference(oc, case, name, rows, opts)
        if d:
            print(d)
            return DIFFERENT
    return 0


if __name__ == "__main__":
    sys.exit(main())
