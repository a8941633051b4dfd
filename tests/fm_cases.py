"""Texts and reads for tests/test_fm_host.py and tests/test_fm_device.py: seeded, made in memory, no files needed.

A case is a FASTA file (bytes) together with what it says: the contigs [(name, comment or None, letters)].
tests/fm_ref.py turns the contigs into the five index files and into search / walk results; scripts/make_golden.py
hands the FASTA bytes to the reference's indexer and keeps what it writes under tests/golden/fm_edges/<name>/.
"""
import gzip
import io

import numpy as np

import fm_ref

LAYOUT_G = [1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2047, 4099]
READ_LENGTHS = [1, 16, 17, 18, 31, 32, 33, 47, 48, 49, 150, 255, 256]
MIN_FIXTURE_G = 15      # the reference's indexer fails below 8 bases and did not finish at 9: shorter texts have no fixture
MIN_READS_G = 64        # texts of 64 bases or more get reads
MAX_WALK_G = 4099       # ... up to the largest layout text (the long-line FASTA case is about the file reader only)
LONG_LINE = 70000
K_PLANT = 24
# the threshold text: (name, forward copies, reverse-complement copies) of a random 24-mer; both strands of the text hold fwd + rev copies
PLANTED = [("k50", 30, 20), ("k52", 26, 26), ("k1", 1, 0), ("k2", 1, 1), ("k3", 2, 1), ("k7", 4, 3), ("k8", 8, 0), ("k9", 5, 4)]


def _rand_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _fasta(contigs, width=60, eol="\n"):
    out = []
    for name, comment, seq in contigs:
        out.append(">" + name + (" " + comment if comment else ""))
        out += [seq[i:i + width] for i in range(0, len(seq), width)]
    return (eol.join(out) + eol).encode()


class Case:
    def __init__(self, name, kind, contigs, fasta=None, gz=False, note=None):
        self.name, self.kind, self.contigs, self.gz, self.note = name, kind, contigs, gz, note
        self.fasta = fasta if fasta is not None else _fasta(contigs)
        self.G = sum(len(c[2]) for c in contigs)
        self.has_fixture = self.G >= MIN_FIXTURE_G
        self.has_reads = MIN_READS_G <= self.G <= MAX_WALK_G
        self.planted = None

    def fasta_file_bytes(self):
        if not self.gz:
            return self.fasta
        buf = io.BytesIO()
        with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0) as fh:
            fh.write(self.fasta)
        return buf.getvalue()

    def files(self):
        """the five files by the plain reference (cached)"""
        if not hasattr(self, "_files"):
            self._files = fm_ref.index_files(self.contigs)
        return self._files

    def text(self):
        if not hasattr(self, "_text"):
            self._text = fm_ref.Text(fm_ref.forward_codes(self.contigs)[0])
        return self._text


def _layout_cases():
    out = []
    for G in LAYOUT_G:
        rng = np.random.default_rng(1000 + G)
        out.append(Case(f"g{G}", "layout", [(f"g{G}", None, _rand_seq(rng, G))]))
    return out


def _fibonacci(n):
    a, b = "A", "AC"
    while len(b) < n:
        a, b = b, b + a
    assert len(b) == n
    return b


def _deep_cases():
    rng = np.random.default_rng(77)
    S = _rand_seq(rng, 777)
    unit = _rand_seq(rng, 37)
    block = _rand_seq(rng, 1500)
    dup = _rand_seq(rng, 53) + block + _rand_seq(rng, 47) + block + _rand_seq(rng, 59)
    texts = [("homopolymer", "A" * 1000), ("at600", "AT" * 600), ("acgt301", "ACGT" * 301), ("palindrome", S + fm_ref.revcomp(S)),
             ("unit37", (unit * 60)[:2201]), ("dup1500", dup), ("fibonacci", _fibonacci(2584))]
    want = {"homopolymer": 1000, "at600": 1200, "acgt301": 1204, "palindrome": 1554, "unit37": 2201, "dup1500": 3159, "fibonacci": 2584}
    for name, seq in texts:
        assert len(seq) == want[name], name
    return [Case(name, "deep", [(name, None, seq)]) for name, seq in texts]


def _threshold_case():
    rng = np.random.default_rng(4242)
    kmers = {name: _rand_seq(rng, K_PLANT) for name, _f, _r in PLANTED}
    copies = []
    for name, fwd, rev in PLANTED:
        copies += [kmers[name]] * fwd + [fm_ref.revcomp(kmers[name])] * rev
    order = rng.permutation(len(copies))
    parts = [_rand_seq(rng, int(rng.integers(3, 10)))]
    for i in order:
        parts += [copies[i], _rand_seq(rng, int(rng.integers(3, 10)))]
    case = Case("threshold", "threshold", [("threshold", "planted 24-mers", "".join(parts))])
    assert case.G <= MAX_WALK_G
    case.planted = {name: (kmers[name], fwd + rev) for name, fwd, rev in PLANTED}
    return case


def _shape_cases():
    rng = np.random.default_rng(99)
    # three contigs of 1, 5 and 4093 bases; a header with a comment and two without; lower case; blank lines
    big = _rand_seq(rng, 4093)
    big = big[:700] + big[700:1300].lower() + big[1300:]
    three = [("one", "a contig of one base", "G"), ("five", None, "ACgtA"), ("big", None, big)]
    lines = [">one a contig of one base", "G", "", ">five", "ACgtA", ">big"]
    for i in range(0, len(big), 70):
        lines.append(big[i:i + 70])
        if i in (140, 2100):
            lines.append("")
    three_fa = ("\n".join(lines) + "\n\n").encode()
    # N runs at a contig's first and last base and across a line break; IUPAC letters side by side; n beside N
    a = "NNNN" + _rand_seq(rng, 52) + "NNNNNNN" + _rand_seq(rng, 100) + "RY" + _rand_seq(rng, 61) + "Nn" + _rand_seq(rng, 40) + "NNN"  # (the 7 N lie over the break at 60)
    b = "n" + _rand_seq(rng, 198) + "K"
    holes = [("runs", "N at both ends", a), ("edge", None, b)]
    # CRLF line ends
    crlf = [("crlf", "carriage returns", _rand_seq(rng, 301)), ("crlf2", None, _rand_seq(rng, 64))]
    # one sequence line longer than the file reader's 64 KiB buffer
    long_line = [("longline", None, _rand_seq(rng, LONG_LINE))]
    return [
        Case("shape_three", "shape", three, fasta=three_fa),
        Case("shape_three_gz", "shape", three, fasta=three_fa, gz=True, note="shape_three"),
        Case("shape_holes", "shape", holes),
        Case("shape_crlf", "shape", crlf, fasta=_fasta(crlf, eol="\r\n")),
        Case("shape_longline", "shape", long_line, fasta=_fasta(long_line, width=LONG_LINE)),
    ]


def all_cases():
    return _layout_cases() + _deep_cases() + [_threshold_case()] + _shape_cases()


_CACHE = {}


def cases():
    """name -> Case, made once per process"""
    if not _CACHE:
        for c in all_cases():
            _CACHE[c.name] = c
    return _CACHE


# ---- reads ------------------------------------------------------------------------------------------
def _piece(text, rng, p, L):
    """L codes of T from p on; random bases where the text has ended"""
    got = text.codes[max(p, 0):max(p, 0) + L] if p < text.N else np.zeros(0, dtype=np.uint8)
    tail = rng.integers(0, 4, L - len(got)).astype(np.uint8)
    return np.concatenate([got, tail]).astype(np.uint8)


def _subst(read, i, rng):
    if i < len(read):
        read[i] = (int(read[i]) + 1 + int(rng.integers(0, 3))) & 3


def reads_for(case):
    """[(tag, codes 0..4 as bytes)] for one text, about 300 of them (cached)"""
    if hasattr(case, "_reads"):
        return case._reads
    text = case.text()
    rng = np.random.default_rng(sum(case.name.encode()) + 31 * case.G)
    N, G = text.N, text.G
    out = []

    def add(tag, codes):
        out.append((tag, bytes(np.asarray(codes, dtype=np.uint8))))

    for L in READ_LENGTHS:
        for _ in range(10):
            add("exact", _piece(text, rng, int(rng.integers(0, max(1, N - L + 1))), L))
        add("at0", _piece(text, rng, 0, L))
        if L >= 2:
            add("junction", _piece(text, rng, max(0, G - L // 2), L))
        if L >= 16:
            add("tail", _piece(text, rng, max(0, N - (L - int(rng.integers(1, L // 2 + 1)))), L))
    for back in (1, 15, 16, 17, 31):
        add("junction", _piece(text, rng, max(0, G - back), 48))
    for L in (32, 150):
        add("to_end", _piece(text, rng, max(0, N - L), L))
    for period in (15, 16, 17, 40):
        for L in (48, 49, 150, 255, 256):
            for _ in range(4):
                r = _piece(text, rng, int(rng.integers(0, max(1, N - L + 1))), L)
                for i in range(period, L, period + 1):  # matching stretches of exactly `period` bases
                    _subst(r, i, rng)
                add(f"subst{period}", r)
    for L in (48, 150, 256):
        for at in (0, 15, 16, 17, 31, 32, 33, L - 1):
            r = _piece(text, rng, int(rng.integers(0, max(1, N - L + 1))), L)
            r[at] = 4
            add(f"n{at}", r)
        for pair in ((15, 16), (31, 32), (16, 32), (0, L - 1)):
            r = _piece(text, rng, int(rng.integers(0, max(1, N - L + 1))), L)
            r[list(pair)] = 4
            add("n2", r)
    add("all_n", np.full(150, 4, dtype=np.uint8))
    add("all_n", np.full(17, 4, dtype=np.uint8))
    if case.name == "dup1500":
        for p in (53, 53 + 1500 - 75, 53 + 1500 + 47 - 20, 53 + 700, 53 + 1547 + 700, 40):
            for L in (150, 256):
                add("repeat", _piece(text, rng, p, L))
    if case.planted:
        code = {"A": 0, "C": 1, "G": 2, "T": 3}
        for name, (kmer, _count) in case.planted.items():
            for k in (kmer, fm_ref.revcomp(kmer)):
                kc = np.array([code[c] for c in k], dtype=np.uint8)
                at = text.bytes.find(bytes(kc), 20)
                assert at >= 20
                lead = _piece(text, rng, at - 20, 20)
                _subst(lead, 19, rng)  # the search before the 24-mer ends on this base: the next one begins on the 24-mer
                add("plant_end", np.concatenate([lead, kc]))                                        # ... and ends with the read
                add("plant_n", np.concatenate([lead, kc, [4], _piece(text, rng, 0, 30)]))           # ... at an N
                add("plant_flank", np.concatenate([lead, _piece(text, rng, at, K_PLANT + 60)]))     # ... somewhere in this copy's flank
                add("plant_only", kc)
    case._reads = out
    return out


def ascii_of(codes: bytes) -> bytes:
    return bytes(b"ACGTN"[c] for c in codes)


def write_index(case, prefix):
    """the five files of the plain reference (byte for byte the reference's own wherever it has made any) as <prefix>.*"""
    for ext, data in case.files().items():
        with open(f"{prefix}.{ext}", "wb") as fh:
            fh.write(data)
    return prefix


def expected_walks(case):
    """per read the (gPos, rPos, len) triples of the plain walk (cached)"""
    if not hasattr(case, "_walks"):
        text = case.text()
        case._walks = [fm_ref.walk(text, codes) for _tag, codes in reads_for(case)]
    return case._walks


def compare_walks(case, n_hits, hits, cap):
    """what a walk entry returned (n_hits[n], hits[n, cap] with gPos / rPos / len) against the plain walk; returns the
    reads that differ as (index, tag, wanted, got) — empty when all agree"""
    bad = []
    for i, ((tag, _codes), want) in enumerate(zip(reads_for(case), expected_walks(case))):
        k = min(len(want), cap)
        got = [(int(h["gPos"]), int(h["rPos"]), int(h["len"])) for h in hits[i, :min(int(n_hits[i]), cap)]]
        if int(n_hits[i]) != len(want) or got != want[:k]:
            bad.append((i, tag, want[:k], got))
    return bad
