"""BAM read input on the GPU: the parser under MCX_READS_BAM (mcx_bam_in.hip) against the sequential restatement of tests/bam_in_vectors.py and against the plain
rule on the FASTQ twin, at chunk sizes 256 and 4 096 and every alignment; a text carried over at every byte; the statuses; mates; and the file front end
(-f reads.bam) on the golden sets against the golden reference SAM and VCF, its ends, its refusals and the command line.

The golden single-end set `se` is FASTA and has no qualities, where a BAM record without qualities stands for a FASTQ record without a quality line (an empty
QUAL column, not '*'): its reads go as records with quality 40, and the SAM is held byte for byte against the run on the FASTQ twin and against the golden
SAM with the QUAL column set aside, as tests/test_bgzf_resident.py does for the same set."""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bam_in_vectors as bv
import test_bam_in_host as th
from conftest import ROOT, VCF_RUNS, VcfOpts, sam_diff, vcf_alg, vcf_body

NEW = ("mcx_bam_reads_header", "mcx_fastq_parser_set_reads", "mcx_fastq_parser_set_mates", "mcx_bam_reads_last", "mcx_bam_reads_last_ms")
EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
G = th.G


# ---- 1. the surface -----------------------------------------------------------------------------------------
def test_the_new_calls_are_declared_bound_and_exported():
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\bint\s+%s\s*\(" % s, header), s
    for name, value in (("MCX_READS_BAM", 2), ("MCX_FASTQ_DAMAGED", 4), ("MCX_FASTQ_UNPAIRED", 5), ("MCX_ROUTE_BAM_IN", 1024)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert (api.READS_BAM, api.FASTQ_DAMAGED, api.FASTQ_UNPAIRED, api.ROUTE_BAM_IN) == (2, 4, 5, 1024)
    assert C.sizeof(api.FastqIn) == 48 and api.FastqIn.n_ref.offset == 44  # (the field lies in what was the struct's tail padding)
    assert "MCX_BAM_CHUNK" in header
    for name in ("set_reads", "set_mates", "bam_last", "bam_last_ms"):
        assert callable(getattr(api.FastqParser, name))
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
        L = api.lib()
        assert L.mcx_fastq_parser_set_mates.argtypes == [C.c_void_p, C.c_int] and L.mcx_bam_reads_last.restype is C.c_int and L.mcx_bam_reads_header.argtypes[1] is C.c_uint64
    main = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()
    assert "BAM input" in main and "BAM input" in open(os.path.join(ROOT, "mapcaller_amd", "run.py")).read()


# ---- the driver ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


def dev_call(api, p, text, max_records, max_read_len, final, n_ref, exp, shift=0, short=None):
    """One mcx_fastq_parse_dev with outputs of exactly the contract's sizes in one tensor, 0xA5 all round, the text `shift` bytes off 16-byte alignment with bytes
    that would make records on either side of it.  (rc, info, outputs as numpy byte arrays with their guards)"""
    import torch
    d = torch.device("cuda", 0)
    room = th.room_of(exp)
    at, total = {}, 0
    for k in th.KEYS:
        at[k] = total
        total += (room[k] + 63) // 64 * 64
    big = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=d)
    base = (-big.data_ptr()) % 64
    side = bv.rd(b"outside", b"ACGT")
    buf = np.frombuffer(side[-(16 + shift):] + bytes(text) + side + bytes(16), dtype=np.uint8).copy()
    tx = torch.from_numpy(buf).to(d)
    assert tx.data_ptr() % 16 == 0
    bufs = {k: big[base + at[k]:base + at[k] + room[k]] for k in th.KEYS}
    fi, fo = th.structs_for(api, lambda x: x.data_ptr(), tx.data_ptr() + 16 + shift, len(text), bufs, exp, max_records, max_read_len, final, n_ref, short)
    info = api.FastqInfo()
    rc = api.lib().mcx_fastq_parse_dev(p._h, C.byref(fi), C.byref(fo), C.byref(info))
    host = big.cpu().numpy()
    return rc, info.as_dict(), {k: host[base + at[k]:base + at[k] + room[k]] for k in th.KEYS}


def twin_outputs(api, fq, twin, exp):
    """the plain rule's outputs on the FASTQ twin, into buffers sized by the BAM call's expectation (they must be the same sizes; max_records one more than the
    reads, so that the stop is the text's own): (info, arrays)"""
    import torch
    d = torch.device("cuda", 0)
    n, info = exp["info"]["n_reads"], exp["info"]
    tx = torch.from_numpy(np.frombuffer(twin + b"\n", dtype=np.uint8).copy()).to(d)
    o = {"bases": torch.zeros(info["n_bases"] + 32, dtype=torch.uint8, device=d), "qual": torch.zeros(info["n_bases"] + 32, dtype=torch.uint8, device=d),
         "off": torch.zeros(n + 2, dtype=torch.int32, device=d), "names": torch.zeros(info["n_name_bytes"] + 1, dtype=torch.uint8, device=d),
         "name_off": torch.zeros(n + 2, dtype=torch.int32, device=d), "rows": torch.zeros((n + 1, exp["row_words"]), dtype=torch.int32, device=d),
         "len": torch.zeros(n + 1, dtype=torch.int32, device=d), "odd": torch.zeros(info["n_odd"] + 1, dtype=torch.int64, device=d)}
    rc, got = fq.parse_dev([tx], n + 1, bv.MAX_LEN, True, text_bytes=[len(twin)], names_cap=info["n_name_bytes"], odd_cap=info["n_odd"], **o)
    assert rc == 0
    return got, {k: v.cpu().numpy() for k, v in o.items()}


def assert_twin(tag, api, fq, text, n_ref, exp):
    """what the BAM call must give is what the plain rule gives on the FASTQ twin: the reads' bases, qualities, names, rows, lengths and odd bytes"""
    twin = bv.twin(text, n_ref)
    if twin is None or exp["info"]["stop"][0] not in (bv.END, bv.EMPTY, bv.TOO_LONG):
        return False
    n = exp["info"]["n_reads"]
    got, o = twin_outputs(api, fq, twin, exp)
    for k in ("n_reads", "longest", "n_odd", "n_bases", "n_name_bytes"):
        assert got[k] == exp["info"][k], (tag, k, got[k], exp["info"][k])
    assert got["stop"][0] == exp["info"]["stop"][0], (tag, got["stop"], exp["info"]["stop"])
    for k, count in (("bases", exp["info"]["n_bases"]), ("qual", exp["info"]["n_bases"]), ("off", n + 1), ("names", exp["info"]["n_name_bytes"]), ("name_off", n + 1),
                     ("len", n), ("odd", exp["info"]["n_odd"])):
        assert o[k].reshape(-1)[:count].tobytes() == np.ascontiguousarray(exp[k]).reshape(-1)[:count].tobytes(), (tag, "twin", k)
    assert o["rows"][:n].tobytes() == exp["rows"].tobytes(), (tag, "twin", "rows")
    return True


def chunks_of(text, chunk):
    return max(1, -(-len(text) // chunk))


# ---- 2. the vectors -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [256, 4096])
def test_parse_dev_equals_the_restatement_and_the_twin_on_every_vector(api, monkeypatch, chunk, capsys):
    monkeypatch.setenv("MCX_BAM_CHUNK", str(chunk))
    twins, report = 0, []
    with api.FastqParser(0) as p, api.FastqParser(0) as fq:
        p.set_reads(api.READS_BAM)
        p.set_rule(api.FASTQ_RULE_GZ)  # (ignored under READS_BAM)
        for name, text, max_len, n_ref in bv.make_vectors():
            big = len(text) // 37 + 1
            exp = bv.restate(text, big, max_len, True, n_ref)
            for shift in range(16):
                rc, info, out = dev_call(api, p, text, big, max_len, True, n_ref, exp, shift)
                assert rc == 0 and info == exp["info"], (name, shift, info, exp["info"])
                th.assert_outputs((name, shift), out, exp)
                last = p.bam_last()
                assert {k: last[k] for k in exp["last"]} == exp["last"] and last["chunks"] == chunks_of(text, chunk), (name, shift, last, exp["last"])
                if shift == 0:
                    report.append((name, last["off_chain"], last["chunks"]))
                    if name == "decoy_%d" % chunk:
                        assert last["off_chain"] >= 1, "the decoy does not test the join: move it"
            twins += assert_twin(name, api, fq, text, n_ref, exp)
            for final, max_records in ((False, big), (True, 2), (False, 1), (True, 0), (True, 3)):
                e = bv.restate(text, max_records, max_len, final, n_ref)
                rc, info, out = dev_call(api, p, text, max_records, max_len, final, n_ref, e)
                assert rc == 0 and info == e["info"], (name, final, max_records, info, e["info"])
                th.assert_outputs((name, final, max_records), out, e)
        assert api.lib().mcx_fastq_parser_set_reads(p._h, 3) == api.ERR_ARG and api.lib().mcx_fastq_parser_set_format(p._h, api.READS_BAM) == api.ERR_ARG  # (set_format keeps to its two)
    assert twins >= 20
    with capsys.disabled():
        print("\n[bam_in] MCX_BAM_CHUNK=%d: (vector, chunks whose searched start was off the chain, chunks) %s" % (chunk, report))


# ---- 3. the carry -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mates", [False, True])
def test_a_text_fed_in_two_parts_at_every_byte(api, monkeypatch, mates):
    """text[:cut] with final = 0, then text[consumed ..) with final = 1: the records put together are the whole text's — six records (three pairs under
    set_mates) and a skipped one between two mates"""
    import torch
    monkeypatch.setenv("MCX_BAM_CHUNK", "256")
    text = th.six_records()
    whole, stop, _ = bv.restate_records(text, 100, bv.MAX_LEN, True, 0, mates)
    assert len(whole) == 6 and stop == bv.END
    whole = np.array([r[:6] for r in whole], dtype=np.int64)
    d = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(d)
    d_recs = torch.zeros(100 * 24, dtype=torch.uint8, device=d)

    def parse(p, lo, hi, final):
        rc, info = p.parse_dev([d_text[lo:hi]], 100, bv.MAX_LEN, final=final, recs=[d_recs], text_bytes=[hi - lo])
        assert rc == 0
        r = d_recs.cpu().numpy().view(np.uint32).reshape(-1, 6)[:info["n_records"][0]].astype(np.int64)
        r[:, [0, 2, 4]] += lo
        return r, info
    with api.FastqParser(0) as p:
        p.set_reads(api.READS_BAM)
        p.set_mates(mates)
        for cut in range(0, len(text) + 1):
            first, info = parse(p, 0, cut, False)
            want = bv.restate_records(text[:cut], 100, bv.MAX_LEN, False, 0, mates)
            assert (info["n_records"][0], info["stop"][0], info["consumed"][0]) == (len(want[0]), want[1], want[2]), (cut, info)
            rest, info2 = parse(p, info["consumed"][0], len(text), True)
            assert info2["stop"][0] == bv.END and np.array_equal(np.concatenate([first, rest]), whole), cut


# ---- 4. the statuses ----------------------------------------------------------------------------------------
def damaged_texts():
    ok = bv.rd(b"ok1", b"ACGTACGTAC") + bv.rd(b"ok2", b"GGATCCN", 0x14)
    after = bv.rd(b"after", b"TTGA")
    good = bv.rd(b"bad", b"ACGTTGCA")
    return [("block_size_too_small", ok + bv.rd(b"bad", b"ACGTTGCA", block_size=len(good) - 4 - 1) + after), ("block_size_negative", ok + bv.rd(b"bad", b"ACGTTGCA", block_size=-8) + after),
            ("block_size_above_2_28", ok + bv.rd(b"bad", b"ACGTTGCA", block_size=(1 << 28) + 1) + after), ("l_read_name_0", ok + bv.rd(b"bad", b"ACGTTGCA", l_read_name=0) + after),
            ("name_without_nul", ok + bv.rd(b"bad", b"ACGTTGCA", nul=b"x") + after), ("last_cut_short", ok + good[:-3]), ("l_seq_negative", ok + bv.rd(b"bad", b"ACGTTGCA", l_seq=-1) + after),
            ("ref_id_beyond_n_ref", ok + bv.rd(b"bad", b"ACGTTGCA", ref=5) + after), ("fixed_part_cut", ok + good[:20])]


@pytest.mark.gpu
def test_the_statuses(api, monkeypatch):
    import torch
    monkeypatch.setenv("MCX_BAM_CHUNK", "256")
    with api.FastqParser(0) as p:
        p.set_reads(api.READS_BAM)
        for name, text in damaged_texts():
            exp = bv.restate(text, 100, bv.MAX_LEN, True, 3)
            assert exp["info"]["stop"][0] == bv.DAMAGED and exp["info"]["n_records"][0] == 2, name
            for shift in (0, 5):
                rc, info, out = dev_call(api, p, text, 100, bv.MAX_LEN, True, 3, exp, shift)
                assert rc == 0 and info == exp["info"], (name, info, exp["info"])
                th.assert_outputs(name, out, exp)
        # two texts
        d = torch.device("cuda", 0)
        t = torch.from_numpy(np.frombuffer(bv.rd(b"a", b"ACGT"), dtype=np.uint8).copy()).to(d)
        rc, info = p.parse_dev([t, t], 10, bv.MAX_LEN)
        assert rc == api.ERR_ARG and b"one text" in api.lib().mcx_last_error() and info["n_reads"] == 0
        # a capacity too small: that group is left alone, the others are complete, and info holds the sizes
        text = dict((n, t) for n, t, _, _ in bv.make_vectors())["letters_odd"]
        exp = bv.restate(text, 100, bv.MAX_LEN, True, 0)
        assert exp["info"]["n_odd"] > 10
        for short, untouched in (("bases_cap", ("bases", "off", "qual")), ("names_cap", ("names", "name_off")), ("odd_cap", ("rows", "len", "odd"))):
            rc, info, out = dev_call(api, p, text, 100, bv.MAX_LEN, True, 0, exp, short=short)
            assert rc == api.ERR_CAPACITY and info == exp["info"], (short, rc, info)
            th.assert_outputs(short, out, exp, untouched)
        # the host form
        rc, info = p.parse([text], 100, bv.MAX_LEN, True)
        assert rc == 0 and info == exp["info"]


# ---- 5. mates -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mates(api, monkeypatch):
    monkeypatch.setenv("MCX_BAM_CHUNK", "256")
    with api.FastqParser(0) as p:
        p.set_reads(api.READS_BAM)
        p.set_mates(True)
        for name, text, stop, pairs in bv.mate_vectors():
            for final in (True, False):
                for cap in (100, 3, 4):
                    exp = bv.restate(text, cap, bv.MAX_LEN, final, 0, True)
                    rc, info, out = dev_call(api, p, text, cap, bv.MAX_LEN, final, 0, exp)
                    assert rc == 0 and info == exp["info"], (name, final, cap, info, exp["info"])
                    th.assert_outputs((name, final, cap), out, exp)
                    if final and cap == 100:
                        assert (info["stop"][0], info["n_records"][0]) == (stop, 2 * pairs), name
        odd = dict((n, t) for n, t, _, _ in bv.mate_vectors())["odd_tail"]
        assert bv.restate_records(odd, 100, bv.MAX_LEN, False, 0, True)[1] == bv.MORE
        # the switch is sticky, and comes off
        p.set_mates(False)
        text = bv.mate_vectors()[2][1]  # swapped: as single reads every record counts
        exp = bv.restate(text, 100, bv.MAX_LEN, True, 0)
        rc, info, out = dev_call(api, p, text, 100, bv.MAX_LEN, True, 0, exp)
        assert rc == 0 and info == exp["info"] and info["n_records"][0] == 6
        assert api.lib().mcx_fastq_parser_set_mates(p._h, 2) == api.ERR_ARG


# ---- 6. the front end ---------------------------------------------------------------------------------------
def fastq_records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def ubam_records(g, name):
    """the golden set's reads as unaligned records, mate by mate (se: FASTA, quality 40 — see the module's note): (records, the FASTQ twin's texts)"""
    if name == "se":
        fa = open(g["r1"], "rb").read().split(b"\n")
        reads = [(h[1:], s, b"I" * len(s)) for h, s in zip(fa[0::2], fa[1::2]) if h]
        recs = [bv.record(n, s, bytes(c - 33 for c in q), 4) for n, s, q in reads]
        return recs, [b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads)]
    a, b = fastq_records(g["r1"]), fastq_records(g["r2"])
    recs = [bv.record(n, s, bytes(c - 33 for c in q), f) for x, y in zip(a, b) for (n, s, q), f in ((x, 0x4D), (y, 0x8D))]
    return recs, [open(g["r1"], "rb").read(), open(g["r2"], "rb").read()]


class Front:
    """an index and a mapper of small batches for a golden set, for several runs"""

    def __init__(self, api, g, max_batch_reads=1 << 13, **kw):
        self.api = api
        self.ix = api.Index(g["prefix"], device=0, full_sa=True)
        self.mp = api.Mapper(self.ix, alg="ksw2", max_batch_reads=max_batch_reads, **kw)

    def run(self, files, out, **kw):
        """(reads or None, error text, output bytes or None, route)"""
        self.mp.reset()
        files = list(files) + [None] * (2 - len(files))
        try:
            st = self.mp.map_files(files[0], files[1], out, **kw)
            return st["reads"], "", open(out, "rb").read() if out else None, self.mp.last_route()
        except self.api.McxError as e:
            return None, str(e), None, self.mp.last_route()

    def close(self):
        self.mp.close(); self.ix.close()


def drop_qual(sam_bytes):
    lines = sam_bytes.decode("latin-1").split("\n")
    return "\n".join("\t".join(f[:10] + ["*"] + f[11:]) if len(f := l.split("\t")) > 10 and not l.startswith("@") else l for l in lines)


def small_launches(monkeypatch):
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    monkeypatch.setenv("MCX_BAM_CHUNK", "1024")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "se"])
def test_front_end_on_unaligned_bam_equals_reference(api, golden, tmp_path, monkeypatch, name):
    """The reads as uBAM in BGZF blocks of 1 000 bytes, a header with @SQ, @RG and @PG lines that are ignored, launches of 64 KB, chunks of 1 KB, batches of 8 192
    reads: the golden SAM byte for byte, whatever the file's name, and the route's new bit."""
    small_launches(monkeypatch)
    g = golden[name]
    recs, twins = ubam_records(g, name)
    path = str(tmp_path / ("reads.bam" if name == "toy" else "reads_without_the_suffix"))
    bv.write_bam(path, recs, [(b"other", 5000)], b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:other\tLN:5000\n@RG\tID:theirs\n@PG\tID:theirs\n", 1000)
    fr = Front(api, g)
    out = str(tmp_path / "bam_in.sam")
    reads, err, sam, route = fr.run([path], out)
    assert err == "" and reads == len(recs), (err, reads)
    want_route = api.ROUTE_INFLATE | api.ROUTE_PARSE | api.ROUTE_ROWS | api.ROUTE_SAM | api.ROUTE_BAM_IN
    assert route == (want_route, 0), route
    if name == "se":
        fq = str(tmp_path / "se.fq")
        open(fq, "wb").write(twins[0])
        twin = fr.run([fq], str(tmp_path / "twin.sam"))
        assert twin[3] == (0, 0) and sam == twin[2]
        assert drop_qual(sam) == drop_qual(open(g["sam"]["ksw2"], "rb").read())
    else:
        nd, ex = sam_diff(g["sam"]["ksw2"], out)
        assert nd == 0, ex
        assert sam == open(g["sam"]["ksw2"], "rb").read()
    # a text file beside it keeps its route and its bytes (no BAM among the inputs: nothing changes)
    plain = fr.run([g["r1"], g["r2"]] if g["r2"] else [g["r1"]], str(tmp_path / "plain.sam"))
    assert plain[3] == (0, 0) and plain[1] == ""
    fr.close()


@pytest.mark.gpu
def test_front_end_on_unaligned_bam_without_sam_gives_the_reference_vcf(api, golden, tmp_path, monkeypatch):
    small_launches(monkeypatch)
    g = golden["var"]
    tag = "default"
    o = VcfOpts(VCF_RUNS[tag][1]).struct
    recs, _ = ubam_records(g, "var")
    path = str(tmp_path / "var.bam")
    bv.write_bam(path, recs, block=1000)
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=vcf_alg("var", tag), max_batch_reads=1 << 13)
    planes = api.planes_alloc(ix.genome_size, "cuda")
    mp.profile_attach(planes.data_ptr(), max_dup=o.max_dup, max_clip=o.max_clip)
    st = mp.map_files(path, None, None)
    assert mp.last_route() == (api.ROUTE_INFLATE | api.ROUTE_PARSE | api.ROUTE_ROWS | api.ROUTE_BAM_IN, 0) and st["reads"] == len(recs)
    mp.profile_finalize(planes.data_ptr())
    out = str(tmp_path / "o.vcf")
    switches = {k: getattr(o, k) for k in ("ploidy", "min_allele_depth", "min_cnv", "min_gap", "fragment_size", "filter", "gvcf", "monomorphic", "somatic")}
    ix.call_variants(planes.data_ptr(), mp.profile_sparse(), st["pairs"], st["pair_dist_sum"], st["pair_len_sum"], out, sample_id=o.sample_id.decode(), ref_name="ref", cmdline="test", **switches)
    got, want = vcf_body(out), vcf_body(g["vcf"][tag])
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:3]
    mp.close(); ix.close()


def sam_to_records(sam_path):
    """the SAM file's lines as aligned BAM records in the file's order, and its references: reversed lines carry reversed bases, CIGARs and tags as they stand"""
    refs, recs = [], []
    for line in open(sam_path, "rb").read().split(b"\n"):
        if line.startswith(b"@SQ"):
            f = dict(x.split(b":", 1) for x in line.split(b"\t")[1:])
            refs.append((f[b"SN"], int(f[b"LN"])))
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        ids = {n: i for i, (n, _) in enumerate(refs)}
        ref = ids.get(f[2], -1)
        nxt = ref if f[6] == b"=" else ids.get(f[6], -1)
        cigar = [] if f[5] == b"*" else [(int(n), op.decode()) for n, op in re.findall(rb"(\d+)([MIDNSHP=X])", f[5])]
        tags = b""
        for t in f[11:]:
            key, typ, val = t.split(b":", 2)
            tags += key + (b"i" + struct.pack("<i", int(val)) if typ == b"i" else b"Z" + val + b"\0")
        seq = b"" if f[9] == b"*" else f[9]
        qual = None if f[10] == b"*" or len(f[10]) != len(seq) else bytes(c - 33 for c in f[10])
        recs.append(bv.record(f[0], seq, qual, int(f[1]), ref, int(f[3]) - 1, int(f[4]), cigar, nxt, int(f[7]) - 1, int(f[8]), tags))
    return recs, refs


@pytest.mark.gpu
def test_remapping_the_golden_sam_gives_the_golden_sam(api, golden, tmp_path, monkeypatch):
    """The golden SAM's own lines as an aligned BAM in input order.  The yardstick is the FASTQ twin: the remapped SAM is byte for byte the SAM of the reads that
    `samtools fastq` would make of the records (0x10: reversed and complemented back).  It is the golden SAM again wherever the golden lines' flags say what
    their SEQ columns hold.  They do not in a few pairs with one unmapped mate, where the reference sets 0x10 | 0x20 on both lines and prints the bases as they
    were sequenced (toy: 13 lines): a reader of BAM has to take the flag at its word, so those pairs' reads come out reverse-complemented and map to the other
    strand.  Those pairs are told apart here by holding the records' reads against the original FASTQ files, and every other line is held to the golden SAM."""
    small_launches(monkeypatch)
    g = golden["toy"]
    recs, refs = sam_to_records(g["sam"]["ksw2"])
    assert len(refs) >= 1 and sum(1 for r in recs if struct.unpack_from("<H", r, 18)[0] & 0x10) > 100
    text = b"".join(recs)
    took, stop, _ = bv.restate_records(text, 1 << 20, 1000, True, len(refs), True)
    assert len(took) == len(recs) and stop == bv.END
    reads = [bv.letters_of(text, r) for r in took]
    original = [x for pair in zip(fastq_records(g["r1"]), fastq_records(g["r2"])) for x in pair]
    odd_pairs = {i >> 1 for i, ((s, q), (_, s0, q0)) in enumerate(zip(reads, original)) if (s, q) != (s0, q0)}
    assert len(odd_pairs) <= 20  # (the reference's quirk, not the rule: see above)
    path = str(tmp_path / "aligned.bam")
    bv.write_bam(path, recs, refs, block=1000)
    twin = [str(tmp_path / "twin_1.fq"), str(tmp_path / "twin_2.fq")]
    for k in (0, 1):
        open(twin[k], "wb").write(b"".join(b"@" + recs[i][36:recs[i].index(b"\0", 36)] + b"\n" + reads[i][0] + b"\n+\n" + reads[i][1] + b"\n" for i in range(k, len(recs), 2)))
    fr = Front(api, g)
    out = str(tmp_path / "remap.sam")
    n_reads, err, sam, route = fr.run([path], out)
    assert err == "" and n_reads == len(recs) and route[0] & api.ROUTE_BAM_IN
    want = fr.run(twin, str(tmp_path / "twin.sam"))
    assert want[1] == "" and sam == want[2]
    got_lines, gold_lines = sam.split(b"\n"), open(g["sam"]["ksw2"], "rb").read().split(b"\n")
    n_head = sum(1 for l in gold_lines if l.startswith(b"@"))
    assert len(got_lines) == len(gold_lines) and got_lines[:n_head] == gold_lines[:n_head]
    differ = [i for i in range(len(recs)) if got_lines[n_head + i] != gold_lines[n_head + i]]
    assert {i >> 1 for i in differ} <= odd_pairs, differ[:5]
    fr.close()


@pytest.mark.gpu
def test_sorted_marked_indexed_output_equals_the_twins(api, golden, tmp_path, monkeypatch):
    small_launches(monkeypatch)
    g = golden["toy"]
    recs, _ = ubam_records(g, "toy")
    path = str(tmp_path / "reads.bam")
    bv.write_bam(path, recs, block=1000)
    fr = Front(api, g)
    kw = dict(bam=True, sort=True, markdup=True, index=True, md=True, mate_tags=True, read_group="@RG\\tID:lane1\\tSM:toy")
    a, b = str(tmp_path / "from_bam.bam"), str(tmp_path / "from_fastq.bam")
    got, want = fr.run([path], a, **kw), fr.run([g["r1"], g["r2"]], b, **kw)
    assert got[1] == "" and want[1] == "" and got[0] == want[0] == len(recs), (got[1], want[1])
    assert got[3][0] & api.ROUTE_BAM_IN and got[3][0] & api.ROUTE_MARKDUP and not want[3][0] & api.ROUTE_BAM_IN
    assert gzip.decompress(got[2]) == gzip.decompress(want[2])
    assert open(a + ".bai", "rb").read() == open(b + ".bai", "rb").read()
    fr.close()


# ---- 7. ends and refusals -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ends_and_refusals(api, golden, tmp_path, monkeypatch, capfd):
    small_launches(monkeypatch)
    g = golden["toy"]
    fr = Front(api, g, max_batch_reads=1000)
    # the golden pairs in coordinate order: the mates are not neighbours
    recs, refs = sam_to_records(g["sam"]["ksw2"])
    key = lambda r: (struct.unpack_from("<i", r, 4)[0] & 0xFFFFFFFF, struct.unpack_from("<i", r, 8)[0])
    by_pos = sorted(recs, key=key)
    assert [r[36:r.index(b"\0", 36)] for r in by_pos[:2]] != [r[36:r.index(b"\0", 36)] for r in recs[:2]]
    path = str(tmp_path / "sorted.bam")
    bv.write_bam(path, by_pos, refs, block=1000)
    out = str(tmp_path / "sorted.sam")
    reads, err, _, _ = fr.run([path], out)
    assert reads is None and "(-2)" in err and "mates are not neighbours" in err and "collate" in err and "sort it by name" in err, err
    # refused before anything is opened
    urecs, _ = ubam_records(g, "toy")
    ubam = str(tmp_path / "reads.bam")
    bv.write_bam(ubam, urecs, block=1000)
    for files in ([g["r1"], ubam], [ubam, g["r2"]], [ubam, ubam]):
        out = str(tmp_path / "refused.sam")
        reads, err, _, _ = fr.run(files, out)
        assert reads is None and "(-5)" in err and "alone" in err and not os.path.exists(out), (files, err)
    fo = api.FileOpts()
    api.lib().mcx_file_opts_default(C.byref(fo))
    fo.shard_count, fo.shard_rank = 2, 0
    out = str(tmp_path / "sharded.sam")
    assert api.lib().mcx_map_files_ex(fr.mp._h, ubam.encode(), None, C.byref(fo), out.encode(), None) == api.ERR_UNSUPPORTED
    assert b"sharded" in api.lib().mcx_last_error() and not os.path.exists(out)
    # a garbage tail: the input ends where the BGZF walk ends it — behind the whole members in front of the garbage — and the record cut there is damaged
    raw = open(ubam, "rb").read()
    cut = raw.find(b"\x1f\x8b\x08\x04", len(raw) // 2)
    garbage = str(tmp_path / "garbage.bam")
    open(garbage, "wb").write(raw[:cut] + b"not a member at all, forty bytes of it.." + raw[cut:])
    text = gzip.decompress(raw[:cut])
    rc, at, n_ref = api.bam_reads_header(text)
    assert rc == 0
    want = bv.restate_records(text[at:], 1 << 20, 1000, True, n_ref, True)
    assert want[1] == bv.DAMAGED and 0 < len(want[0]) < len(urecs)
    capfd.readouterr()
    out = str(tmp_path / "garbage.sam")
    reads, err, sam, _ = fr.run([garbage], out)
    assert err == "" and reads == len(want[0]), (err, reads, len(want[0]))
    said = capfd.readouterr().err
    assert said.count("garbage.bam") == 1 and "behind %d reads" % len(want[0]) in said, said
    assert open(g["sam"]["ksw2"], "rb").read().startswith(sam)
    # a read longer than the context takes, and one without bases: as for FASTQ
    long_recs = urecs[:40] + [bv.rd(b"toolong", b"ACGT" * 300, 0x4D), bv.rd(b"toolong", b"ACGT" * 10, 0x8D)] + urecs[40:]
    bv.write_bam(str(tmp_path / "long.bam"), long_recs, block=1000)
    reads, err, _, _ = fr.run([str(tmp_path / "long.bam")], str(tmp_path / "long.sam"))
    assert reads is None and "read toolong is longer than max_read_len" in err, err
    empty_recs = urecs[:40] + [bv.rd(b"nothing", b"", 0x4D), bv.rd(b"nothing", b"ACGT", 0x8D)] + urecs[40:]
    bv.write_bam(str(tmp_path / "empty.bam"), empty_recs, block=1000)
    reads, err, sam, _ = fr.run([str(tmp_path / "empty.bam")], str(tmp_path / "empty.sam"))
    assert err == "" and reads == 40 and open(g["sam"]["ksw2"], "rb").read().startswith(sam)
    fr.close()


# ---- 8. the command line ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_bam_input(golden, tmp_path):
    g = golden["toy"]
    recs, _ = ubam_records(g, "toy")
    path = str(tmp_path / "reads.bam")
    bv.write_bam(path, recs)
    a, b = str(tmp_path / "from_bam.sam"), str(tmp_path / "from_fastq.sam")
    env = dict(os.environ, MCX_TIMING="1")
    r = subprocess.run([EXE, "-i", g["prefix"], "-f", path, "-alg", "ksw2", "-sam", a, "-no_vcf"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "file 1 %d, file 2 0" % (1 | 2 | 4 | 8 | 1024) in r.stderr and "paired-end" in r.stderr, r.stderr[-2000:]
    r2 = subprocess.run([EXE, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", "ksw2", "-sam", b, "-no_vcf"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert open(a, "rb").read() == open(b, "rb").read()
    usage = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"BAM input" in usage.stdout + usage.stderr
