"""BAM read input: a uBAM writer (struct + zlib: BGZF members with the BC field at a chosen block size), a sequential restatement in Python of the rules as
include/mcx.h words them ("BAM read input"), the FASTQ twin (the text `samtools fastq` would make of the records), and the vectors of tests/test_bam_in_host.py
and tests/test_bam_in_device.py.  Nothing here is taken from the code under test."""
import struct
import zlib

import numpy as np

MORE, END, EMPTY, TOO_LONG, DAMAGED, UNPAIRED = 0, 1, 2, 3, 4, 5
NIB = b"=ACMGRSVTWYHKDBN"
COMP = bytes.maketrans(b"=ACMGRSVTWYHKDBN", b"=TGKCYSBAWRDMHVN")  # the complement of a 4-bit code is its bit reversal
OPS = "MIDNSHP=X"
MAX_LEN = 300  # the vectors' max_read_len


# ---- the writer ---------------------------------------------------------------------------------------------
def tag_z(key, value):
    return key + b"Z" + value + b"\0"


def tag_bc(key, payload):
    return key + b"Bc" + struct.pack("<i", len(payload)) + payload


def record(name, seq, qual=None, flag=4, ref=-1, pos=-1, mapq=0, cigar=(), next_ref=-1, next_pos=-1, tlen=0, tags=b"", block_size=None, l_read_name=None,
           l_seq=None, n_cigar=None, nul=b"\0"):
    """one BAM record: seq as letters in the stored orientation, qual raw Phred bytes (None: 0xFF all through), cigar [(length, op letter)]; the last
    keywords overwrite a field with a value that does not fit the bytes (damaged records)"""
    seq = bytes(seq)
    packed = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= NIB.index(c) << (4 if i % 2 == 0 else 0)
    q = b"\xff" * len(seq) if qual is None else bytes(qual)
    assert len(q) == len(seq)
    cig = b"".join(struct.pack("<I", (n << 4) | OPS.index(op)) for n, op in cigar)
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1 if l_read_name is None else l_read_name, mapq, 4680, len(cigar) if n_cigar is None else n_cigar, flag,
                       len(seq) if l_seq is None else l_seq, next_ref, next_pos, tlen) + name + nul + cig + bytes(packed) + q + tags
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def header(refs=(), text=b""):
    """the BAM header: magic, l_text, text, n_ref, and per reference l_name, name with its NUL, l_ref"""
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs)) + b"".join(struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", l) for n, l in refs)


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf(data, block=0xff00, level=6, eof=True):
    out = []
    for i in range(0, len(data), block):
        chunk = data[i:i + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = c.compress(chunk) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out) + (BGZF_EOF if eof else b"")


def write_bam(path, records, refs=(), text=b"", block=0xff00):
    with open(path, "wb") as f:
        f.write(bgzf(header(refs, text) + b"".join(records), block))


# ---- the rules, restated sequentially ------------------------------------------------------------------------
def header_span(line):
    """the header rule (IdentifyHeaderBegPos / IdentifyHeaderEndPos) on a header line with its newline: (p1, name length)"""
    n = len(line)
    lim = min(n, 100)
    p1 = next((i for i in range(1, n) if line[i] not in b">@"), n - 1)
    p2 = next((i for i in range(1, lim) if line[i] <= 0x20 or line[i] == 0x2F or line[i] >= 0x7F), lim - 1)
    return p1, max(p2 - p1, 0)


def look(text, o, n_ref):
    """what lies at offset o of the chain: ("end",), ("past",), ("bad",) or ("ok", block_size, l_read_name, n_cigar, flag, l_seq); a field is looked at only
    when it lies inside the text"""
    if o >= len(text):
        return ("end",)
    if o + 36 > len(text):
        return ("past",)
    block_size, ref, _, lrn, _, _, n_cig, flag, l_seq, next_ref, _, _ = struct.unpack_from("<iiiBBHHHiiii", text, o)
    if l_seq < 0 or lrn < 1 or block_size > (1 << 28) or 32 + lrn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > block_size:
        return ("bad",)
    if not (-1 <= ref < n_ref and -1 <= next_ref < n_ref):
        return ("bad",)
    nul = o + 36 + lrn - 1
    if nul >= len(text):
        return ("past",)
    if text[nul] != 0:
        return ("bad",)
    if o + 4 + block_size > len(text):
        return ("past",)
    return ("ok", block_size, lrn, n_cig, flag, l_seq)


def chain(text, n_ref):
    """the whole chain: [(offset, block_size, l_read_name, n_cigar, flag, l_seq)], how it stops ("end" / "past" / "bad") and where"""
    out, o = [], 0
    while True:
        r = look(text, o, n_ref)
        if r[0] != "ok":
            return out, r[0], o
        out.append((o,) + r[1:])
        o += 4 + r[1]


def restate_records(text, max_records, max_read_len, final, n_ref=0, mates=False):
    """(records as (name, name_len, seq, rlen, qual, q_take, flag), stop, consumed) by the sequential walk"""
    cap = max_records & ~1 if mates else max_records
    recs, o, consumed, pending = [], 0, 0, None
    while True:
        if pending is None and len(recs) >= cap:
            return recs, MORE, consumed
        r = look(text, o, n_ref)
        if r[0] == "end":
            return recs, (END if pending is None else (UNPAIRED if final else MORE)), consumed
        if r[0] == "past":
            return recs, (DAMAGED if final else MORE), consumed
        if r[0] == "bad":
            return recs, DAMAGED, consumed
        _, block_size, lrn, n_cig, flag, l_seq = r
        nxt = o + 4 + block_size
        if flag & 0x900:
            o = nxt
            if pending is None:
                consumed = o
            continue
        if l_seq == 0:
            return recs, EMPTY, consumed
        if l_seq > max_read_len:
            return recs, TOO_LONG, consumed
        p1, name_len = header_span(b"@" + text[o + 36:o + 36 + lrn - 1] + b"\n")
        seq = o + 36 + lrn + 4 * n_cig
        qual = seq + (l_seq + 1) // 2
        rec = (o + 36 + p1 - 1, name_len, seq, l_seq, qual, 0 if text[qual] == 0xFF else l_seq, flag)
        if not mates:
            recs.append(rec)
            o = consumed = nxt
        elif pending is None:
            pending, o = rec, nxt
        else:
            a, b = pending, rec
            if a[6] & 0x41 != 0x41 or b[6] & 0x81 != 0x81 or text[a[0]:a[0] + a[1]] != text[b[0]:b[0] + b[1]]:
                return recs, UNPAIRED, consumed
            recs += [a, b]
            pending, o = None, nxt
            consumed = nxt


def letters_of(text, rec):
    """(bases as letters, qualities as FASTQ bytes or b"") of a record as sequenced"""
    _, _, seq, rlen, qual, q_take, flag = rec
    s = bytes(NIB[(text[seq + (i >> 1)] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(rlen))
    q = bytes(min(x, 93) + 33 for x in text[qual:qual + q_take])
    if flag & 0x10:
        s, q = s.translate(COMP)[::-1], q[::-1]
    return s, q


def pack_rows(seqs, row_words):
    """mcx_fastq.h's packing rule: A 0, C 1, G 2, T 3, sixteen bases to a word, the first in the top bits; every other letter code 0 and in the odd list, in
    (read, position) order, as (read << 32 | position << 8 | letter)"""
    rows = np.zeros((len(seqs), row_words), dtype=np.uint32)
    odd = []
    for r, s in enumerate(seqs):
        for i, c in enumerate(s):
            k = b"ACGT".find(c)
            if k < 0:
                odd.append((r << 32) | (i << 8) | c)
            else:
                rows[r, i >> 4] |= k << (30 - 2 * (i & 15))
    return rows, np.array(odd, dtype=np.uint64)


def outputs_of(seqs, quals, names, row_words):
    """the call's output groups from the reads' letters, FASTQ quality bytes (b"": none) and names"""
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    rows, odd = pack_rows(seqs, row_words)
    return {"bases": np.frombuffer(b"".join(seqs), dtype=np.uint8), "qual": np.frombuffer(b"".join(q + bytes(len(s) - len(q)) for s, q in zip(seqs, quals)), dtype=np.uint8),
            "names": np.frombuffer(b"".join(names), dtype=np.uint8), "off": np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint32),
            "name_off": np.concatenate([[0], np.cumsum([len(n) for n in names], dtype=np.uint64)]).astype(np.uint32), "rows": rows, "len": lens, "odd": odd,
            "row_words": row_words}


def restate(text, max_records, max_read_len, final, n_ref=0, mates=False, row_words=None):
    """every output of the call as a dict of numpy arrays, "info" as mcx_fastq_info's dict, and "last": mcx_bam_reads_last's first four (of the whole chain)"""
    recs, stop, consumed = restate_records(text, max_records, max_read_len, final, n_ref, mates)
    both = [letters_of(text, r) for r in recs]
    out = outputs_of([s for s, _ in both], [q for _, q in both], [text[r[0]:r[0] + r[1]] for r in recs], (max(max_read_len, 0) + 15) // 16 if row_words is None else row_words)
    out["recs"] = [np.array([r[:6] for r in recs], dtype=np.uint32).reshape(-1, 6)]
    n = len(recs)
    out["info"] = {"n_records": [n, 0], "stop": [stop, 0], "consumed": [consumed, 0], "n_reads": n, "longest": int(out["len"].max()) if n else 0, "n_odd": len(out["odd"]),
                   "n_bases": len(out["bases"]), "n_name_bytes": len(out["names"])}
    ch, _, _ = chain(text, n_ref)
    took = [c for c in ch if not c[4] & 0x900]
    out["last"] = {"walked": len(ch), "taken": len(took), "skipped": len(ch) - len(took), "first_flag": took[0][4] if took else 0}
    return out


# ---- the FASTQ twin -----------------------------------------------------------------------------------------
def twin(text, n_ref=0):
    """The FASTQ text `samtools fastq` would make of the chain's taken records: @read_name, the bases and qualities as sequenced.  A record without qualities
    (0xFF) has no FASTQ form that the plain rule reads as "no quality" unless it is the text's last (its quality line is left out): None for a text with such a
    record elsewhere, and for a name the twin's lines cannot hold (a newline in it)."""
    ch, _, _ = chain(text, n_ref)
    took = [c for c in ch if not c[4] & 0x900]
    out = []
    for k, (o, _, lrn, n_cig, flag, l_seq) in enumerate(took):
        name = text[o + 36:o + 36 + lrn - 1]
        seq = o + 36 + lrn + 4 * n_cig
        qual = seq + (l_seq + 1) // 2
        no_q = l_seq > 0 and text[qual] == 0xFF
        if b"\n" in name or (no_q and k != len(took) - 1):
            return None
        s, q = letters_of(text, (0, 0, seq, l_seq, qual, 0 if no_q else l_seq, flag))
        out.append(b"@" + name + b"\n" + s + b"\n+\n" + (b"" if no_q else q + b"\n"))
    return b"".join(out)


# ---- the vectors --------------------------------------------------------------------------------------------
def rd(name, seq, flag=4, **kw):
    """a record with qualities 30 + position % 10"""
    return record(name, seq, bytes(30 + i % 10 for i in range(len(seq))), flag, **kw)


def filler(size, k=0):
    """an unmapped record of exactly `size` bytes (>= 60), block_size included: a Z tag makes up the length"""
    base = rd(b"fill%d" % k, b"ACGTTGCA")
    assert size >= len(base) + 4, size
    return rd(b"fill%d" % k, b"ACGTTGCA", tags=tag_z(b"XF", b"f" * (size - len(base) - 4)))


def up_to(text, target, k=0):
    """text + fillers so that the next record begins at byte `target`"""
    while len(text) < target:
        left = target - len(text)
        size = left if left <= 700 or left - 600 < 60 else 600
        text += filler(size, k)
        k += 1
    assert len(text) == target
    return text


def decoy_text(boundary):
    """A record that begins 50 bytes before `boundary` and carries a B:c tag whose payload — from boundary + 6 on — is the bytes of three whole valid records: a chunk
    that begins on `boundary` finds its first plausible start inside the tag, off the chain."""
    inner = rd(b"inner1", b"ACGTAC") + rd(b"inner2", b"GGCCTTAA") + rd(b"inner3", b"TTTT")
    t = up_to(rd(b"first", b"ACGTACGTAC"), boundary - 50)
    big = rd(b"decoy", b"ACGT", tags=tag_bc(b"XB", inner))
    assert big.index(inner) == 56
    return t + big + rd(b"after1", b"ACGTTTGA") + rd(b"after2", b"CCGGA")


def make_vectors():
    """[(name, records text, max_read_len, n_ref)]"""
    acgt = b"ACGTTGCAGGATCCAT"
    v = []
    lens = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151, MAX_LEN)
    v.append(("lengths", b"".join(rd(b"len%d" % n, (acgt * 20)[:n]) for n in lens), MAX_LEN, 0))
    v.append(("lengths_reversed", b"".join(rd(b"rev%d" % n, (acgt * 20)[:n], 4 | 0x10) for n in lens), MAX_LEN, 0))
    v.append(("too_long", rd(b"a", b"ACGT") + rd(b"big", (acgt * 20)[:MAX_LEN + 1]) + rd(b"c", b"GG"), MAX_LEN, 0))
    v.append(("empty_seq", rd(b"a", b"ACGT") + rd(b"none", b"") + rd(b"c", b"GG"), MAX_LEN, 0))
    for tag, flag in (("", 4), ("_reversed", 0x14)):
        v.append(("letters_even" + tag, rd(b"all16", NIB, flag) + rd(b"twice", NIB + NIB[::-1], flag), MAX_LEN, 0))
        v.append(("letters_odd" + tag, rd(b"all15", NIB[:15], flag) + rd(b"all17", NIB + b"N", flag) + rd(b"n33", b"N" * 33, flag), MAX_LEN, 0))
    names = [b"n", b"nm", b"x" * 98, b"y" * 99, b"z" * 100, b"w" * 254, b"pair/1", b"two words", b"hi\x7fgh", b"hi\x80gh", b"@@lead", b"@", b"tab\there"]
    v.append(("names", b"".join(rd(n, b"ACGTAC") for n in names), MAX_LEN, 0))
    v.append(("qualities", record(b"q94", b"ACGTACGT", bytes([10, 20, 93, 94, 255, 0, 40, 41])) + record(b"q94r", b"ACGTACG", bytes([10, 20, 93, 94, 255, 0, 40]), 0x14)
              + record(b"noq_last", b"ACGTA"), MAX_LEN, 0))
    v.append(("no_qualities_in_the_middle", record(b"noq", b"ACGTA") + rd(b"after", b"GGCC") + record(b"noq_rev", b"ACGTAN", None, 0x14) + rd(b"last", b"TT"), MAX_LEN, 0))
    sec = [rd(b"sec%d" % i, b"ACGTACGTACGTACGT", 0x100 if i % 2 else 0x800) for i in range(220)]  # 13 KB of them: whole chunks
    v.append(("skipped_first", sec[0] + rd(b"a", b"ACGT") + rd(b"b", b"GGA"), MAX_LEN, 0))
    v.append(("skipped_last", rd(b"a", b"ACGT") + rd(b"b", b"GGA") + sec[1] + sec[2], MAX_LEN, 0))
    v.append(("skipped_run", rd(b"a", b"ACGT") + b"".join(sec) + rd(b"b", b"GGA") + sec[3] + rd(b"c", b"TTGA"), MAX_LEN, 0))
    v.append(("skipped_only", b"".join(sec[:5]), MAX_LEN, 0))
    v.append(("empty", b"", MAX_LEN, 0))
    # chunk boundaries, for chunks of 256 and of 4 096 bytes alike: a record boundary on byte 4096, and a block_size that straddles it by 1, 2 and 3 bytes
    for k in (0, 1, 2, 3):
        t = up_to(rd(b"first", b"ACGTACGTAC"), 4096 - k)
        v.append(("boundary_minus_%d" % k, t + rd(b"at", b"ACGTTGCA" * 5) + rd(b"next", b"GGCCN") + rd(b"last", b"TTAAC", 0x14), MAX_LEN, 0))
    v.append(("longer_than_four_chunks", rd(b"a", b"ACGT") + rd(b"big", b"ACGTN", tags=tag_bc(b"XB", bytes(17000))) + rd(b"b", b"GGA") + rd(b"c", b"TTGAC"), MAX_LEN, 0))
    v.append(("decoy_256", decoy_text(512), MAX_LEN, 0))
    v.append(("decoy_4096", decoy_text(4096), MAX_LEN, 0))
    # aligned records: reference ids, CIGARs, mates' fields
    v.append(("aligned", rd(b"m1", b"ACGTACGTAC", 0x63, ref=0, pos=100, mapq=60, cigar=[(10, "M")], next_ref=2, next_pos=300, tlen=210)
              + rd(b"m1", b"GGATCCATGG", 0x93, ref=2, pos=300, mapq=60, cigar=[(3, "S"), (7, "M")], next_ref=0, next_pos=100, tlen=-210, tags=b"NMC\0"), MAX_LEN, 3))
    return v


def mate_vectors():
    """[(name, records text, expected stop with final = 1, pairs taken)] for set_mates(1)"""
    def pair(k, n1=None, n2=None, f1=0x4D, f2=0x8D):
        return rd(b"p%d" % k if n1 is None else n1, b"ACGTACGTA", f1) + rd(b"p%d" % k if n2 is None else n2, b"GGATCCN", f2)
    sec = rd(b"p1", b"ACGT", 0x100 | 0x4D)
    good = pair(0) + pair(1) + pair(2)
    return [("good", good, END, 3), ("secondary_between", pair(0) + rd(b"p1", b"ACGTACGTA", 0x4D) + sec + rd(b"p1", b"GGATCCN", 0x8D) + pair(2), END, 3),
            ("swapped", pair(0) + pair(1, f1=0x8D, f2=0x4D) + pair(2), UNPAIRED, 1), ("names_differ", pair(0) + pair(1, n2=b"q1") + pair(2), UNPAIRED, 1),
            ("slash_names", pair(0, b"p0/1", b"p0/2") + pair(1, b"p1/1", b"p1/2"), END, 2), ("unpaired_among_pairs", pair(0) + rd(b"p1", b"ACGTACGTA", 0x4C) + rd(b"p1", b"GGATCCN", 0x8D), UNPAIRED, 1),
            ("second_without_0x1", pair(0) + pair(1, f2=0x8C), UNPAIRED, 1), ("odd_tail", good + rd(b"p3", b"ACGTACGTA", 0x4D), UNPAIRED, 3),
            ("odd_tail_then_skipped", good + rd(b"p3", b"ACGTACGTA", 0x4D) + sec, UNPAIRED, 3), ("skipped_after_pairs", good + sec + sec, END, 3)]
