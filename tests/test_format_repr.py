"""repr(float) in integer arithmetic (svim_amd/csrc/fmt_repr.hpp through svx_format_repr / svx_format_repr_many, host only): equal to CPython's repr for every
double tried, no case left out and no tolerance.  The samples are the ones the BED / signature-VCF lines meet (scores, standard deviations) and the ones the
algorithm and the layout can get wrong (random bit patterns, the decimal-exponent boundaries of the layout, powers of two and ten with their neighbours,
subnormals, the extremes)."""
import math
import random
import statistics
import sys

import numpy as np

import helpers as H
from svim_amd import _lib


def _check(values):
    x = np.ascontiguousarray(values, dtype=np.float64)
    got = _lib.format_repr_many(x)
    want = [repr(v) for v in x.tolist()]
    if got != want:
        bad = [(w, g) for w, g in zip(want, got) if w != g]
        raise AssertionError("%d of %d differ, first: repr %s, got %s" % (len(bad), len(want), bad[0][0], bad[0][1]))
    return len(want)


def test_single_call_and_layout_examples():
    for text in ("90.0", "0.0001", "9999999999999998.0", "1e+16", "9.999e-05", "9.223372036854776e+18", "5e-324", "-0.0", "0.0", "inf", "-inf", "nan", "0.1",
                 "0.30000000000000004", "1.7976931348623157e+308", "2.2250738585072014e-308", "123456.785", "1e-05", "1e+22", "1e+23", "-1.5e-10", "1.0", "100.0"):
        assert _lib.format_repr(float(text)) == text == repr(float(text))
    assert _lib.format_repr(float.fromhex("0x1.fffffffffffffp+1023")) == repr(sys.float_info.max)
    assert _lib.format_repr(-float("nan")) == "nan"


def test_two_million_random_bit_patterns():
    rng = np.random.default_rng(20240607)
    bits = rng.integers(0, 2 ** 64, size=2_000_000, dtype=np.uint64)
    x = bits.view(np.float64)
    assert np.isnan(x).sum() > 0                      # NaN payloads are part of the sample: all print as nan
    assert _check(x) == 2_000_000


def test_random_mantissas_at_the_layout_boundaries():
    rng = np.random.default_rng(7)
    for bound in (1e-5, 1e-4, 1e15, 1e16, 1e17, 1e21, 1e22, 1e23):
        scale = rng.uniform(0.05, 20.0, size=200_000)
        x = bound * scale                             # a decade and more on both sides of the boundary, random mantissas
        near = np.nextafter(bound, np.where(rng.integers(0, 2, size=2000) > 0, np.inf, -np.inf))
        for _ in range(6):
            near = np.concatenate([near, np.nextafter(near, np.inf), np.nextafter(near, -np.inf)])[:50_000]
        _check(np.concatenate([x, -x[:1000], near]))


def test_powers_of_two_and_ten_with_neighbours():
    vals = []
    for e in range(-1074, 1024):
        v = math.ldexp(1.0, e)
        vals += [v, math.nextafter(v, math.inf), math.nextafter(v, 0.0)]
    for e in range(-323, 309):
        v = float("1e%d" % e)
        vals += [v, math.nextafter(v, math.inf), math.nextafter(v, 0.0)]
    _check(vals + [-v for v in vals])


def test_subnormals_and_extremes():
    rng = random.Random(3)
    sub = [5e-324 * k for k in range(1, 2000)] + [float.fromhex("0x0.%013xp-1022" % rng.getrandbits(52)) for _ in range(50_000)]
    edge = [sys.float_info.max, -sys.float_info.max, sys.float_info.min, math.nextafter(sys.float_info.min, 0.0), 0.0, -0.0, float("inf"), -float("inf"),
            float("nan"), 5e-324, -5e-324, float(2 ** 53), float(2 ** 53 + 2), 9007199254740993.0, 1e16 - 2, 0.1 + 0.2]
    _check(sub + edge)


def test_hundredths_and_eighths():
    _check([k / 100 for k in range(100_000)])
    _check([k / 8 for k in range(100_000)])
    _check([-k / 100 for k in range(1, 5000)])


def test_standard_deviations_of_small_integer_lists():
    rng = random.Random(11)
    vals = []
    for _ in range(50_000):
        n = rng.randrange(2, 12)
        base = rng.randrange(0, 250_000_000)
        data = [base + rng.randrange(-500, 500) for _ in range(n)]
        vals.append(statistics.stdev(data))
        vals.append(statistics.mean(data))
    _check(vals)


def test_scores_like_calculate_score():
    # n + a * (n / 8) + b * (n / 8) with a, b = 1 - min(1, std / span) (src/svim/SVIM_clustering.py:183-211)
    rng = random.Random(5)
    vals = []
    for n in range(1, 81):
        for _ in range(300):
            span = rng.randrange(40, 100_000)
            a = 1 - min(1, rng.random() * 2 * span / span)
            b = 1 - min(1, statistics.stdev([rng.randrange(0, 2 * span) for _ in range(3)]) / span)
            vals.append(n + a * (n / 8) + b * (n / 8))
    _check(vals)


def _numbers(obj, out):
    if isinstance(obj, float):
        out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _numbers(v, out)
    elif isinstance(obj, list):
        for v in obj:
            _numbers(v, out)


def test_every_score_and_deviation_of_the_goldens():
    g = H.load("g_bed_cases.json.gz")
    vals = []
    for case in g["cases"]:
        _numbers(case["clusters"], vals)
        _numbers(case["candidates"], vals)
    assert len(vals) > 500
    _check(vals)
    # the reference's own files of a real clustering: the name column TYPE[_source;locus];size;std_span;std_pos and the score column, as text
    w = H.load("g_writers.json.gz")
    texts = []
    for name, text in w["files"].items():
        if not name.endswith(".bed"):
            continue
        for line in text.splitlines():
            f = line.split("\t")
            fields = f[3].split(";")
            texts.append(f[4])
            if not fields[0].endswith("_dest"):
                texts += [t for t in fields[-2:] if t != "None"]
    assert len(texts) > 1000
    got = _lib.format_repr_many([float(t) for t in texts])
    assert got == texts
