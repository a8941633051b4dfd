#!/usr/bin/env python3
"""Generates tests/golden/opt/: the reference's output at non-default -indel (MaxPosDiff) and -maxmm (MaxMisMatchRate).

Runs only where oracle/_ref/MapCaller and oracle/_ref/mcref_tool exist (``make -C oracle ref``).  One small genome with
repeats, tandem runs and N runs; a donor with SNPs and insertions / deletions of 1..90 bases; three read sets with 3 % substitutions
per base (so that the -maxmm gate decides for many reads): 150 bp pairs, 250 bp pairs (FASTQ) and single-end reads as FASTA.
Every set is mapped by ``MapCaller -t 1`` with both -alg values at every setting of SETTINGS.

What is kept
------------
<set>.<alg>.default.sam.gz   the default run's SAM in full
<set>.<alg>.<tag>.diff.gz    every other run as the lines that differ from the default run: ``<0-based index among all lines of the
                             SAM>\\t<line>``; SEQ and QUAL of a line are written ``=`` where both equal the default line's (most
                             differing lines are the same read placed elsewhere).  tests/test_options.py rebuild_sam() undoes it.
pe150.ksw2.indel60.m.extra.gz  the further lines of ``-m -indel 60``, in the form of scripts/make_golden_multi.py, against the
                             rebuilt indel60 SAM
pe150.vcf.<tag>.gz           the VCF of ``-vcf`` at -indel 60 and at -maxmm 0.1 (ksw2), without the two header lines that hold paths
pe150.ksw2.indel60.prof.gz / .maps.gz   mcref_tool's dump of the alignment profile and the sparse maps after Mapping() at -indel 60
MANIFEST.json                per run the number of lines, the number that differ from the default run, and the fact that -indel 150
                             gave the -indel 100 SAM (the reference clamps, main.cpp:251-253)

    python scripts/make_golden_opts.py
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mapcaller_amd import synth  # noqa: E402

REF_BIN = os.path.join(ROOT, "oracle", "_ref", "MapCaller")
REF_TOOL = os.path.join(ROOT, "oracle", "_ref", "mcref_tool")
OUT = os.path.join(ROOT, "tests", "golden", "opt")
SKIP = 3000  # keep clear of the genome start, where the reference's mate rescue crashes

# tag -> (-indel, -maxmm) as handed to the command line (None: the option is left out)
SETTINGS = {
    "default": (None, None),
    "indel0": (0, None), "indel10": (10, None), "indel60": (60, None), "indel100": (100, None),
    "maxmm0": (None, "0"), "maxmm0.02": (None, "0.02"), "maxmm0.1": (None, "0.1"),
    "indel60_maxmm0.1": (60, "0.1"), "indel100_maxmm0.1": (100, "0.1"),
}
# name -> (pairs or reads, read length, paired, fastq, seed, substitutions per base: one rate for each equal part of the set).  The 250 bp pairs are
# half at 1.5 %, half at 4.5 % (3 % on average): at a flat 3 % nearly every such read has more seeds than the straight-line path takes and at
# -maxmm 0.02 not one pair would be left to it, and at a flat 2 % -maxmm 0.1 would change next to nothing.
READ_SETS = {"pe150": (1300, 150, True, True, 43, (0.03,)), "pe250": (800, 250, True, True, 44, (0.015, 0.045)), "se": (1000, 250, False, False, 45, (0.03,))}
MIN_DIFF = 0.02  # every non-default run must differ from its default run in at least this share of its lines


def flags(tag):
    indel, mm = SETTINGS[tag]
    return (["-indel", str(indel)] if indel is not None else []) + (["-maxmm", mm] if mm is not None else [])


def gz_write(path, data: bytes):
    with open(path, "wb") as raw:  # mtime=0 keeps the files reproducible
        with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as fh:
            fh.write(data)


def sh(*cmd):
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def sam_lines(data: bytes):
    assert data.endswith(b"\n")
    return data[:-1].split(b"\n")


def diff_lines(base, other):
    """[(index, line of `other` with SEQ / QUAL as '=' where both are the base line's)] for the lines that differ"""
    assert len(base) == len(other), (len(base), len(other))
    out = []
    for i, (a, b) in enumerate(zip(base, other)):
        if a == b:
            continue
        fa, fb = a.split(b"\t"), b.split(b"\t")
        if len(fa) > 10 and len(fb) > 10 and fa[9:11] == fb[9:11]:
            fb[9] = fb[10] = b"="
        out.append((i, b"\t".join(fb)))
    return out


def split_extras(unique, multi):
    """scripts/make_golden_multi.py's: (body of the -m SAM, body of the unique-mode SAM) -> [(index of the primary line, extra line)]"""
    out, u = [], -1
    for line in multi:
        if u + 1 < len(unique) and line == unique[u + 1]:
            u += 1
            continue
        assert u >= 0 and line.split(b"\t", 1)[0] == unique[u].split(b"\t", 1)[0], (u, line[:80])
        out.append((u, line))
    assert u == len(unique) - 1, (u, len(unique))
    return out


def body(lines):
    return [l for l in lines if l and not l.startswith(b"@")]


def main():
    if not (os.path.exists(REF_BIN) and os.path.exists(REF_TOOL)):
        sys.exit("build the reference first: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    manifest = {"settings": {t: flags(t) for t in SETTINGS}, "sets": {}, "runs": {}, "min_diff_share": MIN_DIFF}
    with tempfile.TemporaryDirectory() as tmp:
        g = synth.random_genome([110000, 70000], seed=41, n_repeats=14, repeat_len=500, tandem=6, n_runs=4)
        fa = os.path.join(tmp, "opt.fa")
        synth.write_fasta(fa, g)
        prefix = os.path.join(tmp, "idx")
        sh(REF_BIN, "index", fa, prefix)
        for ext in ("bwt", "sa", "pac", "ann", "amb"):
            shutil.copy(f"{prefix}.{ext}", os.path.join(OUT, f"idx.{ext}"))
        gz_write(os.path.join(OUT, "genome.fa.gz"), open(fa, "rb").read())
        donor = synth.mutate_genome(g, 42, snp=0.004, indel=0.002, max_indel=90)
        log = ["-t", "1", "-log", os.path.join(tmp, "job.log")]
        for name, (n, rlen, paired, fastq, seed, sub) in READ_SETS.items():
            frag = dict(frag_mean=rlen + 300, frag_sd=60, frag_min=rlen + 40, frag_max=rlen + 700) if paired else {}
            bases = torch.cat([synth.simulate_reads(donor, n // len(sub), rlen, paired, seed + 100 * k, skip_head=SKIP, sub=rate, **frag)[0]
                               for k, rate in enumerate(sub)])
            ext = "fq" if fastq else "fa"
            f1, f2 = os.path.join(tmp, f"{name}.r1.{ext}"), os.path.join(tmp, f"{name}.r2.{ext}")
            writer = synth.write_fastq if fastq else synth.write_fasta_reads
            writer(f1, bases, 0, 2 if paired else 1)
            gz_write(os.path.join(OUT, f"{name}.r1.{ext}.gz"), open(f1, "rb").read())
            files = ["-f", f1]
            if paired:
                writer(f2, bases, 1, 2)
                gz_write(os.path.join(OUT, f"{name}.r2.{ext}.gz"), open(f2, "rb").read())
                files += ["-f2", f2]
            manifest["sets"][name] = {"reads": 2 * n if paired else n, "rlen": rlen, "paired": paired, "fastq": fastq, "sub": list(sub)}

            def run(alg, extra, to):
                sh(REF_BIN, "-i", prefix, *files, "-alg", alg, "-sam", to, "-no_vcf", *log, *extra)
                return sam_lines(open(to, "rb").read())

            for alg in ("nw", "ksw2"):
                base = run(alg, [], os.path.join(tmp, "d.sam"))
                gz_write(os.path.join(OUT, f"{name}.{alg}.default.sam.gz"), b"\n".join(base) + b"\n")
                runs = {}
                for tag in SETTINGS:
                    if tag == "default":
                        continue
                    runs[tag] = run(alg, flags(tag), os.path.join(tmp, "o.sam"))
                    d = diff_lines(base, runs[tag])
                    share = len(d) / len(base)
                    print(f"{name} {alg} {tag}: {len(d)} of {len(base)} lines differ ({100 * share:.1f} %)", flush=True)
                    assert share >= MIN_DIFF, "a run that hardly differs from the default: change the donor or the error rates"
                    gz_write(os.path.join(OUT, f"{name}.{alg}.{tag}.diff.gz"), b"".join(b"%d\t%s\n" % x for x in d))
                    manifest["runs"][f"{name}.{alg}.{tag}"] = {"lines": len(base), "differ": len(d)}
                clamp = run(alg, ["-indel", "150"], os.path.join(tmp, "c.sam"))
                assert clamp == runs["indel100"], "-indel 150 is not the -indel 100 run"
                manifest["runs"][f"{name}.{alg}.indel100"]["equals_indel150"] = True
                if (name, alg) == ("pe150", "ksw2"):
                    multi = run(alg, ["-indel", "60", "-m"], os.path.join(tmp, "m.sam"))
                    extras = split_extras(body(runs["indel60"]), body(multi))
                    assert extras
                    gz_write(os.path.join(OUT, f"{name}.{alg}.indel60.m.extra.gz"), b"".join(b"%d\t%s\n" % x for x in extras))
                    manifest["multi"] = {f"{name}.{alg}.indel60": len(extras)}
            if name == "pe150":
                for tag in ("indel60", "maxmm0.1"):
                    vcf = os.path.join(tmp, "o.vcf")
                    sh(REF_BIN, "-i", prefix, *files, "-alg", "ksw2", "-vcf", vcf, *log, *flags(tag))
                    keep = [l for l in open(vcf, "rb").read().split(b"\n") if not l.startswith((b"##command_line=", b"##reference="))]
                    gz_write(os.path.join(OUT, f"{name}.vcf.{tag}.gz"), b"\n".join(keep))
                    manifest.setdefault("vcf", {})[f"{name}.ksw2.{tag}"] = sum(1 for l in keep if l and not l.startswith(b"#"))
                reply = subprocess.run([REF_TOOL], input=f"L {prefix}\nO 60 0.05\nP ksw2 {tmp}/prof {f1} {f2}\n", text=True, stdout=subprocess.PIPE,
                                       stderr=subprocess.DEVNULL, check=True).stdout.split("\n")
                assert reply[0].startswith("ok") and reply[1:3] == ["ok", "ok"], reply
                gz_write(os.path.join(OUT, f"{name}.ksw2.indel60.prof.gz"), open(f"{tmp}/prof.prof", "rb").read())
                gz_write(os.path.join(OUT, f"{name}.ksw2.indel60.maps.gz"), open(f"{tmp}/prof.maps", "rb").read())
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    sizes = {f: os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT)}
    print(f"tests/golden/opt: {len(sizes)} files, {sum(sizes.values())} bytes, largest {max(sizes.values())}")


if __name__ == "__main__":
    main()
