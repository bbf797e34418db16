"""Rows of an interleaved A/B (one bench run per row: `<variant> ms 16.7 collect 2.0 gather 0.19 ...`) -> per variant and column the median and the min-max
range, and for the step time the verdict of the rule the project measures by: a side is faster only if its median beats the other's by more than the larger
of the two ranges.   python tools/ab_table.py TABLE [baseline variant]"""
import statistics
import sys


def main():
    rows = {}
    for line in open(sys.argv[1]):
        f = line.split()
        if len(f) < 3 or line.startswith("#") or f[1] != "ms":
            continue
        rows.setdefault(f[0], []).append({f[i]: float(f[i + 1]) for i in range(1, len(f) - 1, 2)})
    base = sys.argv[2] if len(sys.argv) > 2 else next(iter(rows))
    cols = list(next(iter(rows.values()))[0])
    for v, rs in rows.items():
        print("%-30s n %d  " % (v, len(rs)) + "  ".join("%s %.3f [%.3f-%.3f]" % (c, statistics.median(r[c] for r in rs), min(r[c] for r in rs), max(r[c] for r in rs))
                                                       for c in cols if c != "wc"))
    b = [r["ms"] for r in rows[base]]
    for v, rs in rows.items():
        if v == base:
            continue
        a = [r["ms"] for r in rs]
        gain, spread = statistics.median(b) - statistics.median(a), max(max(a) - min(a), max(b) - min(b))
        print("%s against %s: median %+.3f ms, larger range %.3f ms -> %s" % (v, base, -gain, spread, "faster" if gain > spread else ("slower" if -gain > spread else "no change")))


if __name__ == "__main__":
    main()
