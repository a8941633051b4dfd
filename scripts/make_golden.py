#!/usr/bin/env python3
"""Generates the golden fixtures under tests/golden/ with the REAL reference.

Runs only in the authoring container: it needs oracle/_ref/ (``make -C oracle ref``, which
compiles /root/reference from its own sources) — the reference itself never travels.  What is
committed are data files: index files written by ``MapCaller index``, seeded synthetic reads,
the SAM the reference prints for them at ``-t 1`` and per-function input/output vectors obtained
through oracle/_ref/mcref_tool (oracle/ref_shim.cpp).

    python scripts/make_golden.py

Sets
----
toy   reference test/ref.fa (70 kb, 1 contig); 1500 pairs x 150 bp sampled from test/mut.fa
mc    synthetic 3-contig genome with dispersed + tandem repeats and N runs; 2000 pairs x 150 bp
se    same genome as mc; 2000 single-end FASTA reads x 100 bp with some N
long  synthetic 2-contig genome; 600 pairs x 250 bp at 1 % sub / 1 % ins / 1 % del per base
Each set has ref.<alg>.sam.gz for nw and ksw2, and for one algorithm ref.<alg>.prof.gz / .maps.gz: the\nalignment profile (10 x u16 per position) and the sparse maps the reference holds after Mapping() with -vcf on.
func  bwt_search.json (queries on the toy index) and dp.json (nw/ksw2 strings, ez.score)
fm_edges  index files (and, for three texts, BWT_Search results) for the small texts of tests/fm_cases.py;
      `python scripts/make_golden.py fm_edges` makes this set alone
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mapcaller_amd import synth  # noqa: E402

REF_BIN = os.path.join(ROOT, "oracle", "_ref", "MapCaller")
REF_TOOL = os.path.join(ROOT, "oracle", "_ref", "mcref_tool")
GOLD = os.path.join(ROOT, "tests", "golden")
SKIP = 3000  # keep clear of the genome start, where the reference's mate rescue crashes


def sh(*cmd):
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def gz_write(path, data: bytes):
    with open(path, "wb") as raw:  # mtime=0 keeps the files reproducible
        with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as fh:
            fh.write(data)


def make_set(name, fasta, donor, n, rlen, paired, seed, fastq=True, profile_alg=None, vcf_runs=(), **kw):
    out = os.path.join(GOLD, name)
    os.makedirs(out, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "idx")
        sh(REF_BIN, "index", fasta, prefix)
        for ext in ("bwt", "sa", "pac", "ann", "amb"):
            shutil.copy(f"{prefix}.{ext}", os.path.join(out, f"idx.{ext}"))
        gz_write(os.path.join(out, "genome.fa.gz"), open(fasta, "rb").read())
        bases, _ = synth.simulate_reads(donor, n, rlen, paired, seed, skip_head=SKIP, **kw)
        ext = "fq" if fastq else "fa"
        f1 = os.path.join(tmp, f"r1.{ext}")
        f2 = os.path.join(tmp, f"r2.{ext}")
        writer = synth.write_fastq if fastq else synth.write_fasta_reads
        if paired:
            writer(f1, bases, 0, 2)
            writer(f2, bases, 1, 2)
            files = ["-f", f1, "-f2", f2]
        else:
            writer(f1, bases, 0, 1)
            files = ["-f", f1]
        gz_write(os.path.join(out, f"r1.{ext}.gz"), open(f1, "rb").read())
        if paired:
            gz_write(os.path.join(out, f"r2.{ext}.gz"), open(f2, "rb").read())
        for alg in ("nw", "ksw2"):
            sam = os.path.join(tmp, f"{alg}.sam")
            sh(REF_BIN, "-i", prefix, *files, "-alg", alg, "-sam", sam, "-no_vcf", "-t", "1", "-log", os.path.join(tmp, "job.log"))
            data = open(sam, "rb").read()
            assert data.count(b"\n") >= (2 * n if paired else n), (name, alg)
            gz_write(os.path.join(out, f"ref.{alg}.sam.gz"), data)
        if profile_alg:
            # what Mapping() leaves behind with -vcf on: MappingRecordArr and the sparse maps
            tool = subprocess.Popen([REF_TOOL], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
            cmd = f"L {prefix}\nP {profile_alg} {tmp}/prof {f1} {f2 if paired else ''}\n"
            reply = tool.communicate(cmd)[0].split()
            assert reply[-1] == "ok", reply
            gz_write(os.path.join(out, f"ref.{profile_alg}.prof.gz"), open(f"{tmp}/prof.prof", "rb").read())
            gz_write(os.path.join(out, f"ref.{profile_alg}.maps.gz"), open(f"{tmp}/prof.maps", "rb").read())
        for tag, alg, extra in vcf_runs:
            # the whole -vcf surface: Mapping() + VariantCalling(); the two header lines that hold paths are dropped
            vcf = os.path.join(tmp, f"{tag}.vcf")
            sh(REF_BIN, "-i", prefix, *files, "-alg", alg, "-vcf", vcf, "-t", "1", "-log", os.path.join(tmp, "job.log"), *extra)
            keep = [l for l in open(vcf, "rb").read().split(b"\n") if not l.startswith((b"##command_line=", b"##reference="))]
            gz_write(os.path.join(out, f"ref.vcf.{tag}.gz"), b"\n".join(keep))
    print("set", name, "done")


def make_io_set():
    """Input-side semantics (GetData.cpp) on the toy reads: interleaved -p input with an odd tail and
    decorated headers, multi-line FASTA, .gz files read directly, two libraries in one run."""
    src, out = os.path.join(GOLD, "toy"), os.path.join(GOLD, "io")
    os.makedirs(out, exist_ok=True)
    r1 = gzip.open(os.path.join(src, "r1.fq.gz"), "rb").read().split(b"\n")
    r2 = gzip.open(os.path.join(src, "r2.fq.gz"), "rb").read().split(b"\n")
    n = len(r1) // 4
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(src, "idx")
        log = ["-t", "1", "-no_vcf", "-log", os.path.join(tmp, "job.log")]
        # 1. interleaved, 2999 records: the last 199-read chunk is mapped as single reads
        recs = []
        for i in range(n):
            for k, r in ((1, r1), (2, r2)):
                recs.append(b"\n".join([r[4 * i] + (b"/%d" % k if i % 3 else b" mate%d extra words" % k), r[4 * i + 1], b"+", r[4 * i + 3]]))
        il = b"\n".join(recs[:2999]) + b"\n"
        open(os.path.join(tmp, "il.fq"), "wb").write(il)
        sh(REF_BIN, "-i", prefix, "-f", os.path.join(tmp, "il.fq"), "-p", "-alg", "ksw2", "-sam", os.path.join(tmp, "il.sam"), *log)
        gz_write(os.path.join(out, "il.fq.gz"), il)
        gz_write(os.path.join(out, "ref.il.sam.gz"), open(os.path.join(tmp, "il.sam"), "rb").read())
        # 2. multi-line FASTA, single end
        fa = []
        for i in range(400):
            seq = r1[4 * i + 1]
            fa.append(b">" + r1[4 * i][1:] + b" len=%d" % len(seq))
            fa += [seq[j:j + 60] for j in range(0, len(seq), 60)]
        ml = b"\n".join(fa) + b"\n"
        open(os.path.join(tmp, "ml.fa"), "wb").write(ml)
        sh(REF_BIN, "-i", prefix, "-f", os.path.join(tmp, "ml.fa"), "-alg", "nw", "-sam", os.path.join(tmp, "ml.sam"), *log)
        gz_write(os.path.join(out, "ml.fa.gz"), ml)
        gz_write(os.path.join(out, "ref.ml.sam.gz"), open(os.path.join(tmp, "ml.sam"), "rb").read())
        # 3. .gz inputs handed over as they are (gzGetNextEntry)
        sh(REF_BIN, "-i", prefix, "-f", os.path.join(src, "r1.fq.gz"), "-f2", os.path.join(src, "r2.fq.gz"), "-alg", "ksw2", "-sam", os.path.join(tmp, "gz.sam"), *log)
        gz_write(os.path.join(out, "ref.gz.sam.gz"), open(os.path.join(tmp, "gz.sam"), "rb").read())
        # 4. two libraries in one run: one SAM stream, avgDist carried over
        half = 4 * 700
        for tag, r in (("1", r1), ("2", r2)):
            open(os.path.join(tmp, f"a{tag}.fq"), "wb").write(b"\n".join(r[:half]) + b"\n")
            open(os.path.join(tmp, f"b{tag}.fq"), "wb").write(b"\n".join(r[half:4 * n]) + b"\n")
        sh(REF_BIN, "-i", prefix, "-f", os.path.join(tmp, "a1.fq"), os.path.join(tmp, "b1.fq"), "-f2", os.path.join(tmp, "a2.fq"), os.path.join(tmp, "b2.fq"),
           "-alg", "ksw2", "-sam", os.path.join(tmp, "lib.sam"), *log)
        gz_write(os.path.join(out, "ref.lib.sam.gz"), open(os.path.join(tmp, "lib.sam"), "rb").read())
    print("set io done")


class RefTool:
    """oracle/_ref/mcref_tool (the real reference's functions behind a line protocol)."""

    def __init__(self, prefix):
        self.p = subprocess.Popen([REF_TOOL], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        assert self.ask(f"L {prefix}").startswith("ok")

    def ask(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        return self.p.stdout.readline().rstrip("\n")

    def search(self, codes, start):
        f = self.ask(f"S {start} " + "".join(str(int(c)) for c in codes)).split()
        return int(f[0]), int(f[1]), [int(x) for x in f[2:]]

    def dp(self, q, t):
        f = self.ask(f"D {q} {t}").split(" ")
        return {"nw": [f[0], f[1]], "ksw2": [f[2], f[3]], "ksw2_score": int(f[4]), "ksw2_ops_rev": f[5]}


def make_func_vectors():
    tool = RefTool(os.path.join(GOLD, "toy", "idx"))
    rng = np.random.default_rng(5)
    genome = synth.read_fasta("/root/reference/test/ref.fa").codes[0].numpy()
    # --- BWT_Search: reads cut from the genome (both strands), a few errors and Ns, random start
    queries = []
    for _ in range(1500):
        L = int(rng.integers(20, 160))
        p = int(rng.integers(0, len(genome) - L))
        s = genome[p:p + L].copy()
        if rng.random() < 0.5:
            s = (3 - s)[::-1].copy()
        for _e in range(int(rng.integers(0, 4))):
            s[int(rng.integers(0, L))] = int(rng.integers(0, 5))
        start = int(rng.integers(0, max(1, L - 18)))
        if s[start] > 3:
            s[start] = 0
        ln, fr, loc = tool.search(s, start)
        queries.append({"seq": "".join("ACGTN"[c] for c in s), "start": start, "len": ln, "freq": fr, "loc": loc})
    # low-complexity queries exercise the freq > 50 / short-match branches
    for s in ("A" * 40, "AC" * 30, "ACGT" * 20):
        ln, fr, loc = tool.search(["ACGT".index(c) for c in s], 0)
        queries.append({"seq": s, "start": 0, "len": ln, "freq": fr, "loc": loc})
    json.dump(queries, open(os.path.join(GOLD, "func", "bwt_search.json"), "w"))
    # --- DP: related string pairs of many shapes
    cases = []

    def mutate(s, rate):
        out = []
        for ch in s:
            u = rng.random()
            if u < rate:
                out.append("ACGT"[int(rng.integers(0, 4))])
            elif u < 2 * rate:
                continue
            elif u < 3 * rate:
                out.append(ch)
                out.append("ACGT"[int(rng.integers(0, 4))])
            else:
                out.append(ch)
        return "".join(out) or "A"

    shapes = [(1, 1), (1, 5), (5, 1), (2, 3), (3, 3), (8, 8), (15, 16), (16, 15), (17, 17), (29, 29), (33, 31),
              (63, 64), (64, 64), (65, 64), (64, 65), (100, 106), (127, 129), (130, 128), (200, 208), (257, 260)]
    for m, n in shapes * 6 + [(int(rng.integers(1, 140)), 0) for _ in range(500)]:
        t = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, max(m, 1)))
        q = mutate(t, float(rng.choice([0.0, 0.02, 0.08, 0.2])))
        if n:
            q = (q * 3)[:m] if len(q) < m else q[:m]
            t2 = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, n))
            t = (t + t2)[:n]
        if rng.random() < 0.1:
            i = int(rng.integers(0, len(q)))
            q = q[:i] + "N" + q[i + 1:]
        if rng.random() < 0.05:
            i = int(rng.integers(0, len(t)))
            t = t[:i] + "N" + t[i + 1:]
        rec = {"q": q, "t": t}
        rec.update(tool.dp(q, t))
        cases.append(rec)
    json.dump(cases, open(os.path.join(GOLD, "func", "dp.json"), "w"))
    print("func vectors done:", len(queries), "searches,", len(cases), "DP cases")


FM_SEARCH_TEXTS = ("threshold", "at600", "palindrome")  # texts whose reads' searches are kept as the reference's BWT_Search gives them


def make_fm_edges():
    """tests/golden/fm_edges/<name>/: the five files `MapCaller index` writes for every text of tests/fm_cases.py that it can
    index, and for a few texts what BWT_Search returns along the greedy walk of each read (searches.json.gz).  Texts the
    indexer cannot take are listed in README.md and stay on the plain restatement (tests/fm_ref.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fm_cases
    out_root = os.path.join(GOLD, "fm_edges")
    shutil.rmtree(out_root, ignore_errors=True)
    os.makedirs(out_root)
    left_out, total = [], 0
    for case in fm_cases.cases().values():
        if not case.has_fixture:
            left_out.append((case.name, case.G, "shorter than 15 bases: the reference's indexer exits with an error below 8 bases and did not finish within 60 s at 9"))
            continue
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "ref.fa.gz" if case.gz else "ref.fa")
            open(fa, "wb").write(case.fasta_file_bytes())
            prefix = os.path.join(tmp, "idx")
            try:
                r = subprocess.run([REF_BIN, "index", fa, prefix], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=60)
                failed = None if r.returncode == 0 and all(os.path.exists(f"{prefix}.{e}") for e in ("bwt", "sa", "pac", "ann", "amb")) else f"exit status {r.returncode}"
            except subprocess.TimeoutExpired:
                failed = "ran past 60 s"
            if failed:
                left_out.append((case.name, case.G, f"the reference's indexer failed on it ({failed})"))
                continue
            if case.note:  # the same text as another case in another wrapping: the files must be that case's, nothing more is kept
                for e in ("bwt", "sa", "pac", "ann", "amb"):
                    assert open(f"{prefix}.{e}", "rb").read() == open(os.path.join(out_root, case.note, f"idx.{e}"), "rb").read(), (case.name, e)
                continue
            dst = os.path.join(out_root, case.name)
            os.makedirs(dst)
            # (the long-line case is about the FASTA reader: its .bwt / .sa, 200 KB, are not kept)
            for e in ("pac", "ann", "amb") if case.G > fm_cases.MAX_WALK_G else ("bwt", "sa", "pac", "ann", "amb"):
                shutil.copy(f"{prefix}.{e}", os.path.join(dst, f"idx.{e}"))
                total += os.path.getsize(os.path.join(dst, f"idx.{e}"))
            if case.name in FM_SEARCH_TEXTS:
                tool = RefTool(prefix)
                recs = []
                for _tag, codes in fm_cases.reads_for(case):
                    found, pos = [], 0
                    while pos < len(codes) - 16:  # IdentifySimplePairs' loop (ReadMapping.cpp:133-150)
                        if codes[pos] > 3:
                            pos += 1
                            continue
                        ln, fr, loc = tool.search(codes, pos)
                        found.append([pos, ln, fr, loc])
                        pos += ln + 1
                    if codes and codes[0] <= 3 and not found:  # (a read too short for the walk: one search all the same)
                        ln, fr, loc = tool.search(codes, 0)
                        found.append([0, ln, fr, loc])
                    recs.append({"seq": "".join("ACGTN"[c] for c in codes), "searches": found})
                tool.p.stdin.close()
                tool.p.wait()
                gz_write(os.path.join(dst, "searches.json.gz"), json.dumps(recs, separators=(",", ":")).encode())
                total += os.path.getsize(os.path.join(dst, "searches.json.gz"))
    with open(os.path.join(out_root, "README.md"), "w") as fh:
        fh.write("# fm_edges\n\nIndex files written by the reference's `index` command for the texts of `tests/fm_cases.py`\n"
                 "(made by `scripts/make_golden.py fm_edges`), and for " + ", ".join(FM_SEARCH_TEXTS) + " the results of its `BWT_Search`\n"
                 "along each read's greedy walk (`searches.json.gz`).  `shape_three_gz` is `shape_three` gzip-compressed and shares its files;\n"
                 "of `shape_longline` (one 70 000-character sequence line) only `.pac`, `.ann` and `.amb` are kept.\n\n"
                 "Texts without files here are held to the plain restatement in `tests/fm_ref.py` alone:\n\n| text | bases | why |\n|---|---|---|\n")
        for name, G, why in left_out:
            fh.write(f"| {name} | {G} | {why} |\n")
    print("fm_edges done:", total, "bytes;", len(left_out), "texts left out:", [n for n, _g, _w in left_out])


def main():
    if not (os.path.exists(REF_BIN) and os.path.exists(REF_TOOL)):
        sys.exit("build the reference first: make -C oracle ref")
    if sys.argv[1:] == ["fm_edges"]:
        return make_fm_edges()
    os.makedirs(os.path.join(GOLD, "func"), exist_ok=True)
    mut = synth.read_fasta("/root/reference/test/mut.fa")
    make_set("toy", "/root/reference/test/ref.fa", mut, 1500, 150, True, seed=7,
             frag_mean=500, frag_sd=87, frag_min=350, frag_max=650, profile_alg="ksw2", vcf_runs=[("default", "ksw2", [])])
    with tempfile.TemporaryDirectory() as tmp:
        g = synth.random_genome([160000, 120000, 90000], seed=11, n_repeats=25, repeat_len=600, tandem=12, n_runs=8)
        fa = os.path.join(tmp, "mc.fa")
        synth.write_fasta(fa, g)
        donor = synth.mutate_genome(g, 12)
        make_set("mc", fa, donor, 2000, 150, True, seed=13, sub=0.01, profile_alg="nw", vcf_runs=[("default", "nw", [])])
        make_set("se", fa, donor, 2000, 100, False, seed=14, fastq=False, n_rate=0.002, profile_alg="ksw2", vcf_runs=[("default", "ksw2", [])])
        g2 = synth.random_genome([150000, 150000], seed=21, n_repeats=8, tandem=4)
        fa2 = os.path.join(tmp, "long.fa")
        synth.write_fasta(fa2, g2)
        make_set("long", fa2, synth.mutate_genome(g2, 22), 600, 250, True, seed=23, sub=0.01, ins=0.01, dele=0.01, profile_alg="ksw2",
                 vcf_runs=[("default", "ksw2", [])])
        # the -vcf surface: SNVs (homozygous and heterozygous), short indels, one inversion, one moved segment, ~30x
        g3 = synth.random_genome([60000, 40000], seed=31, n_repeats=6, repeat_len=500, tandem=3)
        fa3 = os.path.join(tmp, "var.fa")
        synth.write_fasta(fa3, g3)
        donor3 = synth.structural_donor(g3, 32)
        make_set("var", fa3, donor3, 10000, 150, True, seed=33, skip_contigs=(0, 2), profile_alg="ksw2",
                 frag_mean=700, frag_sd=40, frag_min=500, frag_max=900,
                 vcf_runs=[("default", "ksw2", []), ("nw", "nw", []), ("gvcf", "ksw2", ["-gvcf"]), ("mono", "ksw2", ["-monomorphic"]),
                           ("filter", "ksw2", ["-filter"]), ("ploidy1", "ksw2", ["-ploidy", "1"]), ("somatic", "ksw2", ["-somatic"]),
                           ("opts", "ksw2", ["-ad", "3", "-min_gap", "20", "-min_cnv", "20", "-size", "400", "-dup", "3", "-maxclip", "10", "-id", "s1"])])
    make_io_set()
    make_func_vectors()
    make_fm_edges()
    torch.manual_seed(0)


if __name__ == "__main__":
    main()
