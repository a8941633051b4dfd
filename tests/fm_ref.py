"""A plain reference for the FM-index files and the seeding searches: numpy and Python only, none of the
product's code.  Everything is restated from the file layouts (bwt.c / bntseq.c of the BWA index the
reference writes) and from what BWT_Search / IdentifySimplePairs compute, in the most direct form that is
still fast enough for texts of a few thousand positions:

* the suffix array by prefix doubling with np.lexsort (a suffix that runs into the end sorts before a
  longer one with the same prefix);
* the BWT with the primary row skipped, occurrence counts every 128 symbols, samples every 32 rows;
* a search that extends while ``bytes.find`` still finds the longer pattern in the text, counts the
  occurrences and orders them by suffix rank.
"""
import numpy as np

OCC_INTERVAL = 128
SA_INTERVAL = 32
MIN_SEED = 16
OCC_THR = 50
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


# ---- the 48-bit generator behind srand48 / lrand48 -----------------------------------------------
class Rand48:
    """X' = (0x5DEECE66D X + 0xB) mod 2^48; srand48(s) sets X = s << 16 | 0x330E; lrand48 gives the top 31 bits."""

    def __init__(self, seed: int):
        self.x = ((seed & 0xFFFFFFFF) << 16) | 0x330E

    def lrand48(self) -> int:
        self.x = (0x5DEECE66D * self.x + 0xB) & ((1 << 48) - 1)
        return self.x >> 17


# ---- suffix array -------------------------------------------------------------------------------
def suffix_array(T) -> np.ndarray:
    """Suffix array of T (codes, any small non-negative integers) without the terminator row."""
    T = np.asarray(T, dtype=np.int64)
    n = len(T)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    rank = T + 1  # 0 is "past the end"
    h = 1
    while True:
        second = np.zeros(n, dtype=np.int64)
        if h < n:
            second[:n - h] = rank[h:]
        order = np.lexsort((second, rank))
        k1, k2 = rank[order], second[order]
        new = np.ones(n, dtype=np.int64)
        new[1:] = 1 + np.cumsum((k1[1:] != k1[:-1]) | (k2[1:] != k2[:-1]))
        rank = np.empty(n, dtype=np.int64)
        rank[order] = new
        if new[-1] == n:
            return order.astype(np.int64)
        h *= 2


def suffix_ranks(sa: np.ndarray) -> np.ndarray:
    rank = np.empty(len(sa), dtype=np.int64)
    rank[sa] = np.arange(len(sa), dtype=np.int64)
    return rank


# ---- the five files -----------------------------------------------------------------------------
def forward_codes(contigs):
    """contigs: [(name, comment or None, sequence text)].  Returns (codes of the concatenated forward genome,
    holes [(offset, length, letter)], per contig (offset, length, holes)): letters outside ACGTacgt become
    lrand48() & 3 of the generator seeded with 11, one draw per letter, in file order."""
    gen = Rand48(11)
    codes, holes, anns = [], [], []
    for _name, _comment, seq in contigs:
        off, n_amb, last = len(codes), 0, None
        for i, ch in enumerate(seq):
            c = "ACGT".find(ch.upper())
            if c < 0:
                if last == ch:
                    holes[-1][1] += 1
                else:
                    holes.append([off + i, 1, ch])
                    n_amb += 1
                c = gen.lrand48() & 3
            last = ch
            codes.append(c)
        anns.append((off, len(seq), n_amb))
    return np.array(codes, dtype=np.uint8), [tuple(h) for h in holes], anns


def text_of(fwd_codes) -> np.ndarray:
    """T = X . revcomp(X)"""
    fwd = np.asarray(fwd_codes, dtype=np.uint8)
    return np.concatenate([fwd, (3 - fwd)[::-1]]).astype(np.uint8)


def _pack2(codes, per_word_bits=32):
    """2-bit codes, first symbol in the top bits, into big-endian-within-word u32 values (zero padded)."""
    n = len(codes)
    n_words = (n + 15) // 16
    padded = np.zeros(n_words * 16, dtype=np.uint64)
    padded[:n] = codes
    shifts = np.array([30 - 2 * s for s in range(16)], dtype=np.uint64)
    return (padded.reshape(n_words, 16) << shifts).sum(axis=1).astype(np.uint32)


def bwt_and_sa_bytes(T, sa=None):
    """(.bwt bytes, .sa bytes) for the text T."""
    T = np.asarray(T, dtype=np.uint8)
    N = len(T)
    if sa is None:
        sa = suffix_array(T)
    rows = np.concatenate([[N], sa]).astype(np.int64)  # row 0 is the terminator's
    primary = int(np.nonzero(rows == 0)[0][0])
    kept = np.delete(rows, primary)
    bwt = T[kept - 1]  # N symbols
    counts = np.bincount(T, minlength=4).astype(np.uint64)
    L2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    words = _pack2(bwt)
    out = []
    running = np.zeros(4, dtype=np.uint64)
    for b in range((N + OCC_INTERVAL - 1) // OCC_INTERVAL):
        out.append(running.copy().tobytes())
        out.append(words[b * 8:(b + 1) * 8].tobytes())
        running += np.bincount(bwt[b * OCC_INTERVAL:(b + 1) * OCC_INTERVAL], minlength=4).astype(np.uint64)
    out.append(running.tobytes())
    head = np.array([primary, L2[1], L2[2], L2[3], L2[4]], dtype=np.uint64).tobytes()
    bwt_bytes = head + b"".join(out)
    n_sa = (N + SA_INTERVAL) // SA_INTERVAL
    samples = rows[np.arange(1, n_sa) * SA_INTERVAL].astype(np.uint64)
    sa_bytes = head + np.array([SA_INTERVAL, N], dtype=np.uint64).tobytes() + samples.tobytes()
    return bwt_bytes, sa_bytes


def index_files(contigs) -> dict:
    """The bytes of .pac .ann .amb .bwt .sa for [(name, comment or None, sequence text)]."""
    fwd, holes, anns = forward_codes(contigs)
    G = len(fwd)
    # .pac: four bases a byte, first in the top bits; then a zero byte if G is a multiple of 4; then G mod 4
    n_bytes = (G + 3) // 4
    padded = np.zeros(n_bytes * 4, dtype=np.uint8)
    padded[:G] = fwd
    q = padded.reshape(n_bytes, 4)
    pac = ((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]).astype(np.uint8).tobytes()
    pac += (b"\0" if G % 4 == 0 else b"") + bytes([G % 4])
    ann = f"{G} {len(contigs)} 11\n"
    for (name, comment, _seq), (off, ln, n_amb) in zip(contigs, anns):
        ann += f"0 {name} {comment if comment else '(null)'}\n{off} {ln} {n_amb}\n"
    amb = f"{G} {len(contigs)} {len(holes)}\n" + "".join(f"{o} {l} {c}\n" for o, l, c in holes)
    bwt, sa = bwt_and_sa_bytes(text_of(fwd))
    return {"pac": pac, "ann": ann.encode(), "amb": amb.encode(), "bwt": bwt, "sa": sa}


# ---- searches -------------------------------------------------------------------------------------
class Text:
    """T with its suffix ranks, for search() and walk()."""

    def __init__(self, fwd_codes):
        self.fwd = np.asarray(fwd_codes, dtype=np.uint8)
        self.G = len(self.fwd)
        self.codes = text_of(self.fwd)
        self.N = len(self.codes)
        self.bytes = self.codes.tobytes()
        self.sa = suffix_array(self.codes)
        self.rank = suffix_ranks(self.sa)


def occurrences(Tb: bytes, pat: bytes, limit=None):
    """start positions of pat in Tb, overlapping ones included; stops after `limit` of them"""
    out, at = [], Tb.find(pat)
    while at >= 0 and (limit is None or len(out) < limit):
        out.append(at)
        at = Tb.find(pat, at + 1)
    return out


def search(text: Text, seq, start: int):
    """BWT_Search(seq, start, len(seq)): (len, freq, locations in suffix order, number of occurrences capped at 51).
    seq: codes 0..4 (bytes or a sequence of ints)."""
    seq = bytes(seq)
    Tb = text.bytes
    pos = start + 1  # the first base is taken whatever it is
    at = Tb.find(seq[start:pos])
    while at >= 0 and pos < len(seq) and seq[pos] <= 3:
        nxt = Tb.find(seq[start:pos + 1], at)  # (an occurrence of the longer pattern is one of the shorter)
        if nxt < 0:
            break
        at = nxt
        pos += 1
    ln = pos - start
    occ = occurrences(Tb, seq[start:pos], OCC_THR + 1)
    if ln >= MIN_SEED and len(occ) <= OCC_THR:
        locs = sorted(occ, key=lambda p: text.rank[p])
        return ln, len(locs), locs, len(occ)
    return ln, 0, [], len(occ)


def walk(text: Text, seq):
    """IdentifySimplePairs' loop before its PosDiff filter: the (gPos, rPos, len) triples in order."""
    seq = bytes(seq)
    out, pos, stop = [], 0, len(seq) - MIN_SEED
    while pos < stop:
        if seq[pos] > 3:
            pos += 1
            continue
        ln, _freq, locs, _n = search(text, seq, pos)
        out.extend((g, pos, ln) for g in locs)
        pos += ln + 1
    return out
