#!/usr/bin/env python3
"""MapCaller's command line on one or several MI355X of a node.

    python -m mapcaller_amd.run -i idx -f r1.fq [-f2 r2.fq] [-alg nw|ksw2] [-sam out.sam [-gpu_sam | -bgzf] | -bam out.bam [-sort [-markdup] [-index]]] [-md] [-rg LINE] [-mc] [-gpu_inflate] [-gpu_gz] [-gpu_parse] [-vcf out.vcf | -no_vcf] ...
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 -m mapcaller_amd.run -i idx -f r1.fq -f2 r2.fq -sam out.sam -vcf out.vcf

One process per GPU.  The input stream is cut into batches that are dealt to the ranks in turn
(reads shard embarrassingly): every rank walks the files, maps its own batches against
its own replica of the index and writes its part of the SAM; rank 0 puts the parts back into input
order.  While they map, the ranks exchange a few KB per round (api.dist_exchange) so that the run
follows the ONE insert-size trajectory and the ONE duplicate-cap order of the input stream: SAM and
VCF equal the single-stream run's.  With -vcf on, the bulk exchange of the run follows
(mapcaller_amd/dist.py): the per-position counter planes are summed onto rank 0 with an RCCL reduce,
the sparse tallies and the run totals gathered, and rank 0 calls the variants (mcx_call_variants).
(The C++ product does the same without Python: mapcaller-mi355x -gpus N.)

Host-side glue only: parsing, mapping, SAM text and variant calling all happen behind the C ABI.
"""
import argparse
import os
import shutil
import sys

import torch

from . import api, dist as mdist


class _Output(argparse.Action):
    """-sam FILE / -bam FILE name the one output file; the switch that comes last says what it holds (reference src/main.cpp:274-285)"""
    def __call__(self, parser, namespace, values, option_string=None):
        namespace.sam = values
        namespace.bam = option_string == "-bam"


def parse(argv):
    ap = argparse.ArgumentParser(prog="mapcaller_amd.run", add_help=True, prefix_chars="-", allow_abbrev=False)
    ap.add_argument("-i", dest="index", required=True, help="BWT index prefix")
    ap.add_argument("-f", dest="f1", nargs="+", required=True, help="files with #1 mates reads (fa, fq, fq.gz; or BAM input, given alone without -f2: the records' flags say whether they are pairs — mates must be neighbours — or single reads; secondary and supplementary records are skipped, reversed ones read as sequenced; inflated, found and unpacked on the GPU, which implies -gpu_inflate -gpu_parse and, with -sam, -gpu_sam; not with several GPUs)")
    ap.add_argument("-f2", dest="f2", nargs="*", default=[], help="files with #2 mates reads")
    ap.add_argument("-p", "-pair", dest="interleaved", action="store_true", help="paired-end reads are interlaced in the same file")
    ap.add_argument("-alg", default="nw", choices=["nw", "ksw2"])
    ap.add_argument("-sam", default=None, action=_Output)
    ap.add_argument("-bam", dest="sam", action=_Output, metavar="FILE", help="BAM output instead of -sam (the later of the two counts): records made and BGZF blocks deflated on the GPU; unsorted, no index; one process only")
    ap.set_defaults(bam=False)
    ap.add_argument("-sort", dest="sort", action="store_true", help="with -bam: a coordinate-sorted BAM file, sorted and merged on the GPU (temporary disk of the file's size beside it, 12 bytes of host memory a record; one library, one process; -index writes its .bai)")
    ap.add_argument("-md", dest="md", action="store_true", help="an MD:Z tag behind XS on every mapped line (what samtools calmd adds), made on the GPU behind each batch's mapping; with every SAM / BAM output; not on several GPUs")
    ap.add_argument("-rg", dest="rg", default=None, metavar="LINE", help="read group, bwa mem -R's form ('@RG\\tID:lane1\\tSM:x'): the line ends the header, RG:Z:<ID> goes on every line; with every SAM / BAM output; not on several GPUs")
    ap.add_argument("-mc", dest="mc", action="store_true", help="MC:Z and MQ:i (the mate's CIGAR and MAPQ) on the lines of pairs whose mate is mapped and whose FLAG has 0x8 clear (what samtools fixmate -m adds); not with -m, not on several GPUs")
    ap.add_argument("-markdup", dest="markdup", action="store_true", help="with -bam -sort: set flag bit 0x400 on duplicate records (pairs by both unclipped 5' ends, single reads by one; the best by base qualities stays), decided on the GPU; 4 more bytes of host memory a record and 24 a pair until the merge; not with -m")
    ap.add_argument("-index", dest="bai", action="store_true", help="with -bam -sort: write the file's index beside it (FILE.bai, what samtools index makes), built on the GPU while the merge writes the file")
    ap.add_argument("-vcf", default="output.vcf")
    ap.add_argument("-no_vcf", action="store_true")
    ap.add_argument("-m", dest="multi", action="store_true", help="a SAM line for every alignment with the best score")
    ap.add_argument("-gpu_sam", dest="gpu_sam", action="store_true", help="make the SAM text on the GPU instead of with host threads (same bytes)")
    ap.add_argument("-bgzf", dest="bgzf", action="store_true", help="write the SAM file as BGZF, its blocks deflated on the GPU (implies -gpu_sam; gzip -d gives the plain file's bytes; one process only)")
    ap.add_argument("-gpu_parse", dest="gpu_parse", action="store_true", help="parse plain FASTQ and plain FASTA read files and pack their reads on the GPU instead of with host threads (same reads)")
    ap.add_argument("-gpu_gz", dest="gpu_gz", action="store_true", help="with -gpu_parse (and -gpu_sam where a SAM file is written): ordinary .gz read files (gzip, pigz; not BGZF) are inflated on the GPU and the reads stay there from the compressed bytes to the SAM text (same reads); files the block-start search cannot cut, and -gpu_gz without -gpu_parse, are read as before")
    ap.add_argument("-gpu_inflate", dest="gpu_inflate", action="store_true", help="inflate BGZF (bgzip) read files on the GPU instead of with host threads (same reads); with -gpu_parse on BGZF FASTQ or FASTA (and -gpu_sam where a SAM file is written) the reads stay on the GPU from the compressed bytes to the SAM text")
    ap.add_argument("-indel", type=int, default=30, help="maximal indel size (MaxPosDiff), at most 100")
    ap.add_argument("-maxmm", type=float, default=0.05, help="maximal mismatch rate in read alignment (MaxMisMatchRate)")
    ap.add_argument("-t", dest="threads", type=int, default=0, help="host threads per process for parsing / SAM text")
    ap.add_argument("-batch", type=int, default=1 << 20, help="reads per batch (the unit dealt to the ranks)")
    ap.add_argument("-maxlen", type=int, default=0, help="longest read the contexts are sized for [sampled from the first reads, 256..1000]")
    for name, kw in (("-gvcf", {}), ("-monomorphic", {}), ("-filter", {}), ("-somatic", {})):
        ap.add_argument(name, action="store_true", **kw)
    ap.add_argument("-ploidy", type=int, default=2)
    ap.add_argument("-size", type=int, default=500)
    ap.add_argument("-ad", type=int, default=5)
    ap.add_argument("-dup", type=int, default=5)
    ap.add_argument("-maxclip", type=int, default=5)
    ap.add_argument("-min_cnv", type=int, default=50)
    ap.add_argument("-min_gap", type=int, default=50)
    ap.add_argument("-id", dest="sample", default="unknown")
    ap.add_argument("-backend", default=None, help="torch.distributed backend (default nccl = RCCL)")
    a = ap.parse_args(argv)
    if a.f2 and len(a.f2) != len(a.f1):
        ap.error("Paired-end reads input numbers do not match!")
    if a.indel > 100:  # main.cpp:251-253
        print("Warning! The maximal indel size is 100!", file=sys.stderr)
        a.indel = 100
    return a


def mapper_kwargs(a):
    """What of the command line goes into every mapping context (api.Mapper)."""
    return dict(alg=a.alg, max_read_len=a.maxlen, max_batch_reads=max(200, a.batch // 200 * 200), multi=a.multi,
                max_pos_diff=a.indel, max_mismatch_rate=a.maxmm)


def sample_read_length(path, lines=40000):
    """Longest sequence line among the first records of a read file (sizes the contexts)."""
    import gzip
    import struct
    with open(path, "rb") as fh:
        bgzf = fh.read(4) == b"\x1f\x8b\x08\x04"
    if bgzf:
        with gzip.open(path, "rb") as fh:
            t = fh.read(4 << 20)  # a BAM file: the header and the first records
        if t[:4] == b"BAM\1":
            rc, o, _ = api.bam_reads_header(t)
            longest = 0
            while rc == 0 and o + 36 <= len(t):
                block_size, l_seq = struct.unpack_from("<i", t, o)[0], struct.unpack_from("<i", t, o + 20)[0]
                if block_size < 32 or l_seq < 0:
                    break
                longest, o = max(longest, l_seq), o + 4 + block_size
            return longest
    opener = gzip.open if path.endswith(".gz") else open
    longest, fastq = 0, False
    with opener(path, "rb") as fh:
        for n, line in enumerate(fh):
            if n >= lines:
                break
            if n == 0:
                fastq = line.startswith(b"@")
            if (n % 4 == 1) if fastq else (not line.startswith(b">")):
                longest = max(longest, len(line.rstrip(b"\r\n")))
    return longest


def main(argv=None):
    a = parse(sys.argv[1:] if argv is None else argv)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.sort and not a.bam:
        sys.exit("-sort puts BAM records into coordinate order: it needs -bam (SAM text is not sorted)")
    if a.bai and not a.sort:
        sys.exit("-index writes the .bai of a coordinate-sorted BAM file: it needs -bam -sort")
    if a.md and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("-md makes its MD tags on one GPU: it cannot be combined with a run on several")
    if (a.rg is not None or a.mc) and world > 1:
        sys.exit("-rg and -mc make their tags on one GPU: they cannot be combined with a run on several")
    if a.mc and a.multi:
        sys.exit("-mc cannot be combined with -m: an extra line is paired with another candidate of the mate than the one whose CIGAR is held")
    if a.markdup and not a.sort:
        sys.exit("-markdup flags the duplicates of a coordinate-sorted BAM file: it needs -bam -sort")
    if a.markdup and getattr(a, "multi", False):
        sys.exit("-markdup takes one record a read: it cannot be combined with -m")
    if a.sort and world > 1:
        sys.exit("-sort sorts and merges on one GPU: it cannot be combined with several ranks")
    if a.bam and world > 1:
        sys.exit("-bam writes one BGZF stream from one GPU: it cannot be combined with several ranks (a sharded BAM writer does not exist yet)")
    if a.bgzf and world > 1:
        sys.exit("-bgzf writes one BGZF stream from one GPU: it cannot be combined with several ranks (a sharded BGZF writer does not exist yet)")
    n_dev = torch.cuda.device_count()
    if n_dev == 0:
        sys.exit("mapcaller_amd.run needs a GPU: the hot path has no CPU fallback")
    device = local % n_dev
    torch.cuda.set_device(device)
    dev = torch.device("cuda", device)
    td = None
    if world > 1:
        import torch.distributed as td_
        td = td_
        backend = a.backend or "nccl"
        td.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))
    if a.maxlen <= 0:
        a.maxlen = min(1000, max(256, (max(sample_read_length(f) for f in a.f1 + a.f2) + 63) // 64 * 64))
    index = api.Index(a.index, device=device, full_sa=True)
    mapper = api.Mapper(index, **mapper_kwargs(a))
    want_vcf = not a.no_vcf
    planes = None
    if want_vcf:
        planes = api.planes_alloc(index.genome_size, dev)
        mapper.profile_attach(planes.data_ptr(), max_dup=a.dup, max_clip=a.maxclip)
    totals = {"reads": 0, "mapped": 0, "pairs": 0, "pair_dist_sum": 0, "pair_len_sum": 0}
    link = api.dist_exchange(dev) if world > 1 else None
    for k, f1 in enumerate(a.f1):  # libraries one after the other, like the reference: one SAM stream, one insert-size state
        f2 = a.f2[k] if a.f2 else None
        # (the ranks write into the one SAM file, every batch's lines at their final place: mcx_map_files_ex)
        st = mapper.map_files(f1, f2, a.sam or None, interleaved=a.interleaved, threads=a.threads,
                              shard=(rank, world) if world > 1 else None, exchange=link, append_sam=k > 0, device_sam=a.gpu_sam, device_inflate=a.gpu_inflate, device_gz=a.gpu_gz, device_parse=a.gpu_parse, bgzf_sam=a.bgzf, bam=a.bam, sort=a.sort, index=a.bai, markdup=a.markdup, md=a.md, read_group=a.rg, mate_tags=a.mc)
        for key in totals:
            totals[key] += st[key]
        if td:
            td.barrier()
    tot = mdist.sum_over_ranks([totals[k] for k in ("reads", "mapped", "pairs", "pair_dist_sum", "pair_len_sum")], dev)
    if want_vcf:
        mapper.profile_settle()  # differences -> counts, before the planes are summed
        planes, sparse = mdist.reduce_profile(planes, mapper.profile_sparse_raw(shard=world > 1), index.genome_size, mapper=mapper)
        if rank == 0:
            mapper.profile_finalize(planes.data_ptr())
            vs = index.call_variants(planes.data_ptr(), sparse, tot[2], tot[3], tot[4], a.vcf, ploidy=a.ploidy, min_allele_depth=a.ad,
                                     min_cnv=a.min_cnv, min_gap=a.min_gap, fragment_size=a.size, filter=int(a.filter), gvcf=int(a.gvcf),
                                     monomorphic=int(a.monomorphic), somatic=int(a.somatic), sample_id=a.sample, ref_name=a.index,
                                     cmdline=" ".join(["mapcaller_amd.run"] + (sys.argv[1:] if argv is None else list(argv))))
            print(f"\t{vs['n_snv']}(snp); {vs['n_ins']}(ins); {vs['n_del']}(del); {vs['n_tnl'] >> 1}(trans); {vs['n_inv'] >> 1}(inversion)", file=sys.stderr)
    if rank == 0:
        kind = "paired-end" if (a.f2 or a.interleaved or tot[2] > 0) else "single-end"  # (BAM input: the records' flags decide)
        print(f"All the {tot[0]} {kind} reads have been processed on {world} GPU(s).\n{tot[1]:12d} reads are mapped properly.\n"
              f"{2 * tot[2]:12d} reads are mapped in pairs.", file=sys.stderr)
    mapper.close()
    index.close()
    if td:
        td.barrier()
        td.destroy_process_group()


if __name__ == "__main__":
    main()
