#!/usr/bin/env python3
"""Generates the -m fixtures: tests/golden/<set>/ref.<alg>.m.extra.gz.

Runs only where oracle/_ref/MapCaller exists (``make -C oracle ref``).  For the committed index and reads
of mc, se, long and var it runs ``MapCaller ... -m -no_vcf -t 1`` and checks that the first line of every
read is the line of the committed unique-mode SAM (ref.<alg>.sam.gz).  Only the further lines are kept,
one per line of the file: ``<0-based index of the read's first line among the SAM lines of ref.<alg>.sam.gz>
\\t<SAM line>`` (header lines not counted).  The tests rebuild the -m SAM from the two files (rebuild_multi
in tests/test_multi.py).

    python scripts/make_golden_multi.py
"""
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "MapCaller")
GOLD = os.path.join(ROOT, "tests", "golden")
SETS = {"mc": ("nw", "ksw2"), "se": ("nw", "ksw2"), "long": ("nw", "ksw2"), "var": ("nw", "ksw2")}


def gz_write(path, data: bytes):
    with open(path, "wb") as raw:  # mtime=0 keeps the files reproducible
        with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as fh:
            fh.write(data)


def body(data: bytes):
    return [l for l in data.split(b"\n") if l and not l.startswith(b"@")]


def split_extras(unique, multi):
    """(multi lines, unique lines) -> [(index of the primary line, extra line)]; asserts that removing the
    extras gives the unique-mode SAM."""
    out, u = [], -1
    for line in multi:
        if u + 1 < len(unique) and line == unique[u + 1]:
            u += 1
            continue
        assert u >= 0 and line.split(b"\t", 1)[0] == unique[u].split(b"\t", 1)[0], (u, line[:80])
        out.append((u, line))
    assert u == len(unique) - 1, (u, len(unique))
    return out


def main():
    if not os.path.exists(REF_BIN):
        sys.exit("oracle/_ref/MapCaller is missing: make -C oracle ref")
    for name, algs in SETS.items():
        d = os.path.join(GOLD, name)
        with tempfile.TemporaryDirectory() as tmp:
            prefix = os.path.join(tmp, "idx")
            for ext in ("bwt", "sa", "pac", "ann", "amb"):
                os.symlink(os.path.join(d, f"idx.{ext}"), f"{prefix}.{ext}")
            reads = []
            for f in ("r1.fq.gz", "r2.fq.gz", "r1.fa.gz"):
                if os.path.exists(os.path.join(d, f)):
                    dst = os.path.join(tmp, f[:-3])
                    open(dst, "wb").write(gzip.open(os.path.join(d, f)).read())
                    reads.append(dst)
            files = ["-f", reads[0]] + (["-f2", reads[1]] if len(reads) > 1 else [])
            for alg in algs:
                sam = os.path.join(tmp, f"{alg}.m.sam")
                subprocess.run([REF_BIN, "-i", prefix, *files, "-alg", alg, "-sam", sam, "-m", "-no_vcf", "-t", "1",
                                "-log", os.path.join(tmp, "job.log")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                unique = body(gzip.open(os.path.join(d, f"ref.{alg}.sam.gz")).read())
                extras = split_extras(unique, body(open(sam, "rb").read()))
                gz_write(os.path.join(d, f"ref.{alg}.m.extra.gz"), b"".join(b"%d\t%s\n" % (i, l) for i, l in extras))
                print(f"{name} {alg}: {len(unique)} -> {len(unique) + len(extras)} lines", flush=True)


if __name__ == "__main__":
    main()
