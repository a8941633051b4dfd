"""The seeded DP problems that tests/test_dp_device.py gives the lane kernels on the GPU and tests/test_hostemu_golden.py gives the
host build of the same headers, and what the oracle (oracle/libmcx_oracle.so: mcxo_nw / mcxo_ksw2 / mcxo_ksw2_extz) says about them.
A plain helper: no fixtures, no product code."""
import ctypes
import random

# the boundary grid: strip edges for K = 8 and 16, the 8 x 8 window edges of the walks, the 16-bases-per-word edges of the staged
# query, the class limits 16 / 32 / 64 / 256
GRID_T = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256]
GRID_Q = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300]
SEED = 20261018
RAGGED_N = [1, 2, 63, 64, 65, 127, 128, 129]


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def descent(rng, max_t=256, max_q=300, n=None):
    """A query and a target that descend from one sequence by substitutions, insertions and deletions (rates 0, 0.02, 0.05, 0.15),
    ragged now and then, an N in one query in ten: what test_two_problems_per_lane_dp_equals_one_per_lane_on_random_shapes draws."""
    n = n or rng.randint(1, max_t)
    t = _rand(rng, n)
    rate = rng.choice([0.0, 0.02, 0.05, 0.15])
    q = []
    for ch in t:
        r = rng.random()
        if r < rate / 3: continue                                   # deletion
        if r < 2 * rate / 3: q.append(rng.choice("ACGT"))            # insertion before
        q.append(rng.choice("ACGT") if rng.random() < rate else ch)  # substitution
    if rng.random() < 0.2: q = q[: rng.randint(1, max(1, len(q)))]   # ragged: a short query against a long target
    if rng.random() < 0.2: q = q + [rng.choice("ACGT") for _ in range(rng.randint(1, 40))]
    q = q[:max_q] or ["A"]
    if rng.random() < 0.1: q[rng.randrange(len(q))] = "N"
    return "".join(q), t


_SET = None


def problem_set():
    """[(query, target)]: the boundary grid (each cell once with unrelated strings, once with the query cut from the target repeated),
    the extremes of the 16-bit argument, 600 random descents.  1149 problems; built once."""
    global _SET
    if _SET is None:
        rng = random.Random(SEED)
        p = []
        for n in GRID_T:
            for m in GRID_Q:
                p.append((_rand(rng, m), _rand(rng, n)))
                t = _rand(rng, n)
                p.append(((t * (m // n + 1))[:m], t))
        p += [("A" * 300, "C" * 256), ("N" * 300, _rand(rng, 256)), ("A" * 1000, "C" * 256), ("N" * 1000, _rand(rng, 256)), ("A" * 2048, "C" * 256),
              ("A" * 1000, "A" * 256), ("A", "A" * 256), ("A" * 300, "A"), ("ACGT" * 75, "ACGT" * 64)]
        p += [descent(rng) for _ in range(600)]
        _SET = p
    return list(_SET)


def for_strip(probs, strip):
    """The one filter: strips of 8 columns take targets of at most 64 bases."""
    return [p for p in probs if strip == 16 or len(p[1]) <= 64]


def unlike_order(probs):
    """The list reordered so that every problem shares a lane of the two-per-lane form once as A (an even place) and once as B (an odd
    place) with a problem a third of the list away.  Returns (the 2 n problems, for each of them its index in probs)."""
    n = len(probs)
    idx = []
    for i in range(n):
        idx += [i, (i + n // 3) % n]
    return [probs[i] for i in idx], idx


def mixed_groups(strip):
    """Groups of 128 (two groups of 64 for the one-per-lane form): one 300 x 256 or 1000 x 256 problem (x 64 for strips of 8) among 127 of
    1 x 1 ... 9 x 9, the large one in the first lane's low half, in a middle lane's high half, and last."""
    rng = random.Random(SEED + 1)
    wide = 256 if strip == 16 else 64
    out = []
    for rows, at in ((300, 0), (1000, 77), (300, 127)):
        g = [(_rand(rng, k), _rand(rng, k)) for k in (1 + i % 9 for i in range(127))]
        q, t = descent(rng, n=wide, max_q=rows)
        g.insert(at, ((q + _rand(rng, rows))[:rows], t))
        out += g
    return out


def wavefront_extras():
    """What the wavefront-per-problem form (mcx_extend_batch: k_extend<1|4|16>) takes beyond the lane forms' limits: targets of 257, 1023 and
    1024 bases, one 2048 x 1024 problem, targets that hold an N — descents all of them."""
    rng = random.Random(SEED + 2)
    p = [descent(rng, n=n, max_q=2048) for n in (257, 1023, 1024)]
    q, t = descent(rng, n=1024, max_q=2048)
    while len(q) < 2048:
        q += _rand(rng, 2048 - len(q))
    p.append((q[:2048], t))
    for n in (5, 40, 100, 300):
        q, t = descent(rng, n=n)
        k = rng.randrange(n)
        p.append((q, t[:k] + "N" + t[k + 1:]))
    return p


# ---- the oracle's answers ------------------------------------------------------------------------------------------------------
def nt4(ch):
    return "ACGT".find(ch.upper()) if ch.upper() in "ACGT" else 4


_ANSWERS = {}


def oracle_gapped(L, alg, q, t):
    """(gapped read string, gapped genome string) of mcxo_nw / mcxo_ksw2; an oracle return below 0 is an error, never a skip."""
    key = (alg, q, t)
    if key not in _ANSWERS:
        cap = len(q) + len(t) + 2
        o1, o2 = ctypes.create_string_buffer(cap), ctypes.create_string_buffer(cap)
        rc = (L.mcxo_nw if alg == "nw" else L.mcxo_ksw2)(q.encode(), len(q), t.encode(), len(t), o1, o2, cap)
        assert rc >= 0, (rc, alg, q, t)
        _ANSWERS[key] = (o1.value.decode(), o2.value.decode())
    return _ANSWERS[key]


def columns(a1, a2):
    """The column string of two gapped strings: 'M' base over base, 'I' a '-' in the genome string, 'D' a '-' in the read string."""
    assert len(a1) == len(a2)
    return "".join("D" if x == "-" else ("I" if y == "-" else "M") for x, y in zip(a1, a2))


def oracle_columns(L, alg, q, t):
    a1, a2 = oracle_gapped(L, alg, q, t)
    assert a1.replace("-", "") == q and a2.replace("-", "") == t
    return columns(a1, a2)


def oracle_ksw2_score(L, q, t):
    """ez.score of ksw_extz2_sse (mcxo_ksw2_extz)."""
    qc, tc = bytes(nt4(c) for c in q), bytes(nt4(c) for c in t)
    sc = ctypes.c_int()
    buf = ctypes.create_string_buffer(len(q) + len(t) + 2)
    assert L.mcxo_ksw2_extz(qc, len(q), tc, len(t), ctypes.byref(sc), buf, len(q) + len(t) + 2) >= 0
    return sc.value


def runs(cols):
    """[(kind, length)] of a column string, in column order."""
    out = []
    for c in cols:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return [(k, n) for k, n in out]


def nw_score2(a1, a2):
    """Twice the score of an alignment under nw_alignment's parameters (nw_alignment.cpp:18-83: match +1, mismatch -1, a gap's first
    column -1.5, every further one -0.5; an N equals nothing but an N), computed from the two gapped strings alone."""
    s = 0
    for k, n in runs(columns(a1, a2)):
        if k != "M":
            s -= 2 + n
    for x, y in zip(a1, a2):
        if x != "-" and y != "-":
            s += 2 if nt4(x) == nt4(y) else -2
    return s


def summary_of(cols, q, t):
    """csrc/mcx_types.h DpSummary of a problem restated from its column string and its two strings alone (definitions: DpSumAcc in
    csrc/mcx_dp_lane.h).  rle: the words in use, in column order (None beyond eight runs, where n_rle is 0xFFFF)."""
    op = {"M": 0, "I": 1, "D": 2}
    rs = runs(cols)
    qi = ti = n = mis = 0
    for c in cols:
        if c == "M":
            n += 1
            mis += 1 if (nt4(q[qi]) > 3 or nt4(q[qi]) != nt4(t[ti])) else 0  # a query N differs from every target base
            qi += 1; ti += 1
        elif c == "I":
            qi += 1
        else:
            ti += 1
    assert qi == len(q) and ti == len(t)
    kinds = [k for k, _ in rs]
    first = kinds.index("M") if "M" in kinds else len(rs)                      # no 'M' at all: the whole string is head and tail alike
    last = len(rs) - 1 - kinds[::-1].index("M") if "M" in kinds else -1
    lead, tail = rs[:first], rs[last + 1:]
    count = lambda part, k: sum(n_ for k_, n_ in part if k_ == k)
    return {
        "cols_off": len(q) + len(t) - len(cols), "cols_len": len(cols), "n": n, "mis": mis, "switches": len(rs),
        "lead_d": count(lead, "D"), "lead_i": count(lead, "I"), "lead_runs": len(lead),
        "tail_d": count(tail, "D"), "tail_i": count(tail, "I"), "tail_runs": len(tail),
        "n_rle": len(rs) if len(rs) <= 8 else 0xFFFF,
        "rle": [(n_ << 4) | op[k_] for k_, n_ in rs] if len(rs) <= 8 else None,
    }
