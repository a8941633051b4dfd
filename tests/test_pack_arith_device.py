"""k_pack_reads with the look-up pack4, 16-byte loads at the reads' own byte addresses and two reads per thread, through the public API on the GPU: whole
and partial 32-base parts, both strands and every load offset in one launch against the oracle; batches whose longest reads (and so the kernel's
workgroup shape and the rows' stride) differ one after the other on one context, a refused batch among them; and the odd-flags form of the kernel
(-vcf) against the walk that does not read those flags."""
import numpy as np
import pytest

from conftest import sam_diff
from test_pack_device import _batch_arrays, _oracle_sam, _rc, _sam_of_batch, _write_fastq, api, mc_genome  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

LENS = (31, 32, 33, 63, 64, 65, 95, 96, 97, 150, 151, 256)
ODD = b"NnacgtRYKMSWBDHV"  # N, lower-case letters, IUPAC letters


def _reads(genome, n_pairs, lens, seed, paired=True):
    """n_pairs pairs (or reads) cut from the genome, mate 2 reverse-complemented 300 further on, their lengths those of `lens` in turn (the mates of a pair
    take different ones); every third read has an N, a lower-case or an IUPAC letter at its first byte, its last byte or byte 15 / 16 / 31 / 32 counted
    from either end"""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    for i in range(n_pairs):
        p = int(rng.integers(2000, len(genome) - 3000))
        mates = [bytearray(genome[p:p + lens[(2 * i if paired else i) % len(lens)]])]
        if paired:
            b = lens[(2 * i + 1) % len(lens)]
            mates.append(bytearray(_rc(genome[p + 300:p + 300 + b])))
        for r in mates:
            if k % 3 == 0:
                n = len(r)
                at = [0, n - 1, 15, 16, 31, 32, n - 16, n - 17, n - 32, n - 33][(k // 3) % 10]
                if 0 <= at < n:
                    r[at] = ODD[(k // 3) % len(ODD)]
            k += 1
            out.append(bytes(r))
    return out


def _oracle_of(prefix, reads, paired, tmp, tag):
    f1, f2, ora = (str(tmp / f"{tag}.{x}") for x in ("r1.fq", "r2.fq", "ora.sam"))
    if paired:
        _write_fastq(f1, reads[0::2]); _write_fastq(f2, reads[1::2])
    else:
        _write_fastq(f1, reads)
    _oracle_sam(prefix, f1, f2 if paired else None, "ksw2", ora)
    return ora


@pytest.fixture(scope="module")
def first_batch(mc_genome):
    return _reads(mc_genome, 256, LENS, seed=3)


def test_whole_and_partial_parts_equal_oracle(api, golden, mc_genome, first_batch, tmp_path):
    """256 pairs and 255 single reads of 31 to 256 bases: parts of 32 whole bases and partial last ones, mate 2 reversed, read starts at every residue
    mod 16, odd letters at the parts' edges — SAM equal to the oracle's."""
    g = golden["mc"]
    ix = api.Index(g["prefix"], device=0)
    for paired, reads in ((True, first_batch), (False, _reads(mc_genome, 255, LENS, seed=4, paired=False))):
        off = np.cumsum([0] + [len(r) for r in reads])
        assert len({int(o) & 15 for o in off[:-1]}) == 16
        assert {len(r) for r in reads} == set(LENS)
        ora = _oracle_of(g["prefix"], reads, paired, tmp_path, f"p{int(paired)}")
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=512)
        out = str(tmp_path / f"gpu.{int(paired)}.sam")
        _sam_of_batch(api, ix, mp, reads, paired, out)
        nd, ex = sam_diff(ora, out, mask_se_reverse_qual=True)
        assert nd == 0, (paired, ex)
        mp.close()
    ix.close()


def test_batches_of_other_longest_reads_one_after_the_other(api, golden, mc_genome, tmp_path):
    """One context, five batches of 64 pairs whose longest reads are 150, 33, 256 (single-end), 150 and 150 bases: rows shorter, longer and as long as
    those of the batch before, workgroups of 5, 2 and 8 parts — each batch's SAM equals the oracle's and what a fresh context gives for it alone.  Then
    a batch with a read longer than max_read_len is refused as ever, and the 150-base batch after it maps as before."""
    g = golden["mc"]
    ix = api.Index(g["prefix"], device=0)
    shapes = [(150, True), (33, True), (256, False), (150, True), (150, True)]
    mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=128)
    texts = []
    for k, (longest, paired) in enumerate(shapes):
        lens = [n for n in LENS if n <= longest]
        reads = _reads(mc_genome, 64, lens, seed=20 + k, paired=paired)
        assert max(len(r) for r in reads) == longest
        ora = _oracle_of(g["prefix"], reads, paired, tmp_path, f"b{k}")
        out, alone = str(tmp_path / f"gpu.{k}.sam"), str(tmp_path / f"alone.{k}.sam")
        mp.reset()  # (the insert-size state: each batch is a run of its own to the oracle)
        _sam_of_batch(api, ix, mp, reads, paired, out)
        nd, ex = sam_diff(ora, out, mask_se_reverse_qual=True)
        assert nd == 0, (k, ex)
        fresh = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=128)
        _sam_of_batch(api, ix, fresh, reads, paired, alone)
        fresh.close()
        assert open(out, "rb").read() == open(alone, "rb").read(), k
        texts.append((reads, paired, open(out, "rb").read()))
    # a read of 300 bases among reads of 150
    reads = list(texts[0][0])
    reads[5] = bytes(mc_genome[5000:5300])
    bases, off = _batch_arrays(reads)
    mp.reset()
    with pytest.raises(api.McxError, match=r"a read of 300 bases is longer than max_read_len \(256\)"):
        mp.map_batch(bases, off, True)
    reads, paired, want = texts[0]
    out = str(tmp_path / "after.sam")
    mp.reset()
    _sam_of_batch(api, ix, mp, reads, paired, out)
    assert open(out, "rb").read() == want
    mp.close(); ix.close()


def test_odd_flags_form_equals_the_column_walk(api, golden, first_batch, monkeypatch):
    """The first test's pairs with the profile attached (-vcf): k_pack_reads then sets a read's odd flag, and the bookkeeping writes the reads without it
    as runs.  With MCX_PROF_BY_COLUMN=1 every read is walked column by column whatever its flag says: the ten planes and the tallies must be the same
    both ways (a flag missing from a read with a lower-case or an IUPAC letter would send that read down the runs' path)."""
    g = golden["mc"]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    bases, off = _batch_arrays(first_batch)
    res = []
    for by_column in (False, True):
        if by_column:
            monkeypatch.setenv("MCX_PROF_BY_COLUMN", "1")
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=512)
        planes = api.planes_alloc(ix.genome_size, "cuda")
        mp.profile_attach(planes.data_ptr())
        for _ in range(2):
            mp.reset()  # (a batch starts on a chunk boundary of the insert-size walk)
            mp.map_batch(bases, off, True)
        mp.profile_finalize(planes.data_ptr())
        sp = mp.profile_sparse_raw().copy()
        sp[:, 10:] *= (np.arange(54)[None, :] < sp[:, 9:10]).astype(np.uint8)  # (a record's bytes past its length are anything)
        res.append((api.planes_view(planes, ix.genome_size).cpu().numpy().copy(), sorted(bytes(x) for x in sp)))
        mp.close()
    ix.close()
    assert int(res[0][0][0:4].sum()) > 10000  # (the reads were counted: some 80 000 bases)
    assert np.array_equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]
