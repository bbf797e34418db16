#!/usr/bin/env python
"""Rate of the genome load: writes a synthetic FASTA of a given size (plain, BGZF, gzip), loads it through the device loader (svx_genome_load_fasta) and through
the Python route (convert.genome_arrays + set_genome), checks that both leave the same genome in the context and prints one JSON line.  One process, one GPU.

    python tools/genome_load_rate.py --mb 1024 --container plain [--contigs 4] [--dir /tmp] [--repeats 3] [--skip-host]
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bgzf_block(payload, level):
    """one BGZF block: raw DEFLATE behind the gzip header with the 'BC' extra field, CRC32 and ISIZE behind it"""
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    cd = comp.compress(payload) + comp.flush()
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(cd) + 25) + cd + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload))


class Writer(object):
    def __init__(self, path, container, level):
        self.fh, self.container, self.level, self.buf = open(path, "wb"), container, level, b""
        self.z = zlib.compressobj(level, zlib.DEFLATED, 31) if container == "gzip" else None

    def write(self, data):
        if self.container == "plain":
            self.fh.write(data)
        elif self.container == "gzip":
            self.fh.write(self.z.compress(data))
        else:
            self.buf += data
            k = 0
            while len(self.buf) - k >= 0xff00:
                self.fh.write(bgzf_block(self.buf[k:k + 0xff00], self.level))
                k += 0xff00
            self.buf = self.buf[k:]

    def close(self):
        if self.container == "gzip":
            self.fh.write(self.z.flush())
        elif self.container == "bgzf":
            if self.buf:
                self.fh.write(bgzf_block(self.buf, self.level))
            self.fh.write(bgzf_block(b"", self.level))
        self.fh.close()


def write_fasta(path, container, total_bytes, n_contig, level, seed=1):
    """lines of 60 bases; the same 16 MB of random lines repeated with a per-chunk rotation (the generator is not what is measured)"""
    rng = np.random.default_rng(seed)
    rows = (16 << 20) // 61
    a = np.empty((rows, 61), dtype=np.uint8)
    a[:, :60] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(rows, 60), dtype=np.uint8)]
    a[:, 60] = 10
    w = Writer(path, container, level)
    per = total_bytes // n_contig
    names = []
    for c in range(n_contig):
        names.append("chr%d" % (c + 1))
        w.write(b">chr%d synthetic contig\n" % (c + 1))
        left = per // 61
        k = 0
        while left > 0:
            n = min(left, rows)
            w.write(np.roll(a, (c * 7 + k) % rows, axis=0)[:n].tobytes())
            left -= n
            k += 1
    w.close()
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=1024.0, help="bytes of FASTA text, in MB")
    ap.add_argument("--container", choices=("plain", "bgzf", "gzip"), default="plain")
    ap.add_argument("--contigs", type=int, default=4)
    ap.add_argument("--level", type=int, default=1, help="deflate level of the generated file")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true", help="do not time the Python route (nor check against it)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from svim_amd import _lib, convert
    d = tempfile.mkdtemp(prefix="svx_genome_", dir=args.dir)
    path = os.path.join(d, "g.fa" + ("" if args.container == "plain" else ".gz"))
    out = {"tool": "genome_load_rate", "container": args.container, "text_MB": args.mb, "contigs": args.contigs}
    try:
        t0 = time.perf_counter()
        names = write_fasta(path, args.container, int(args.mb * 1e6), args.contigs, args.level)
        out["write_s"] = time.perf_counter() - t0
        out["file_bytes"] = os.path.getsize(path)
        eng = _lib.Engine(args.device)
        refs = names[::-1]
        runs = []
        for _ in range(args.repeats):                       # (the first run also pays the staging buffers and the page cache)
            t0 = time.perf_counter()
            off, st = eng.load_genome_fasta(path, refs)
            st["wall_s"] = time.perf_counter() - t0
            runs.append(st)
        best = min(runs, key=lambda r: r["wall_s"])
        out["device"] = best
        out["device_first_run_wall_s"] = runs[0]["wall_s"]
        out["device_text_MB_per_s"] = best["raw_bytes"] / 1e6 / best["wall_s"]
        import resource
        out["max_rss_MB_after_device_route"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
        if not args.skip_host:
            d_off, d_codes = eng.fetch_genome()
            os.environ["SVX_GENOME_HOST"] = "1"
            t0 = time.perf_counter()
            h_off, hst = convert.load_genome(eng, path, refs)
            out["host"] = dict(hst, wall_s=time.perf_counter() - t0)
            del os.environ["SVX_GENOME_HOST"]
            g_off, g_codes = eng.fetch_genome()
            out["equal"] = bool(np.array_equal(d_off, g_off) and np.array_equal(d_codes, g_codes) and np.array_equal(off, h_off))
            out["speedup"] = out["host"]["wall_s"] / best["wall_s"]
            out["max_rss_MB_after_host_route"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
        eng.close()
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(d)
    print(json.dumps(out))
    return 0 if out.get("equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
